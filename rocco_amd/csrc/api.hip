// rocco_amd/csrc/api.hip -- C ABI entry points of librocco_hip.so (see include/rocco_hip.h).
#include <map>
#include <memory>
#include <mutex>
#include "kernels.h"
#include <atomic>

#include "budget.h"
#include "inflate_core.h"
#include "bigwig_sections.h"
#include "fragments_rules.h"

#include <algorithm>
#include <cmath>
#include <new>

namespace rocco {

static thread_local std::string g_last_error;

void set_last_error(const std::string &msg) { g_last_error = msg; }

// How often a solver buffer had to grow (hipMalloc + hipFree, or the pinned twins): the count path's batch sizes every
// buffer of a pipeline before its worker threads start, so that no thread allocates or frees device memory -- both
// device-wide synchronisations -- while the others' streams are in flight (tests/test_gpu_count_path_batch.py reads this).
static std::atomic<long long> g_buffer_growths{0};

int DeviceBuffer::reserve(size_t want)
{
    if (want <= bytes) {
        return ROCCO_HIP_OK;
    }
    g_buffer_growths.fetch_add(1, std::memory_order_relaxed);
    // small buffers double (few growths); large ones take what is asked for + 1/16 -- a 40 GB scratch must not become 80 --
    // and the old block goes first (nothing is carried over: a scratch buffer's contents end with the call that wrote them)
    size_t grow = bytes ? bytes * 2 : (size_t)1 << 16;
    if (grow < want || want >= ((size_t)256 << 20)) {
        grow = want + ((want >= ((size_t)256 << 20)) ? want / 16 : 0);
    }
    if (ptr != nullptr) {
        (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    void *p = nullptr;
    ROCCO_HIP_TRY(hipMalloc(&p, grow));
    ptr = p;
    bytes = grow;
    return ROCCO_HIP_OK;
}

void DeviceBuffer::release()
{
    if (ptr != nullptr) {
        (void)hipFree(ptr);
    }
    ptr = nullptr;
    bytes = 0;
}

SharedFactor::~SharedFactor() { buf.release(); }

int PinnedBuffer::reserve(size_t want)
{
    if (want <= bytes) {
        return ROCCO_HIP_OK;
    }
    g_buffer_growths.fetch_add(1, std::memory_order_relaxed);
    size_t grow = bytes ? bytes * 2 : (size_t)1 << 14;
    if (grow < want) {
        grow = want;
    }
    void *p = nullptr;
    ROCCO_HIP_TRY(hipHostMalloc(&p, grow, coherent ? (hipHostMallocCoherent | hipHostMallocMapped) : hipHostMallocDefault));
    if (ptr != nullptr) {
        (void)hipHostFree(ptr);
    }
    ptr = p;
    bytes = grow;
    return ROCCO_HIP_OK;
}

void PinnedBuffer::release()
{
    if (ptr != nullptr) {
        (void)hipHostFree(ptr);
    }
    ptr = nullptr;
    bytes = 0;
}

}  // namespace rocco

using namespace rocco;

// What the record entry points (count.hip, interval_count.hip, fragment_length.hip) do once their arguments have passed:
// the solver's device, no other library's stale error for this call's launch checks, `bytes` of dev_misc (0: the launcher's
// *_scratch_bytes refused the shape).
static int enter_record_call(rocco_hip_solver *solver, size_t bytes)
{
    if (bytes == 0) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device));
    (void)hipGetLastError();
    return solver->dev_misc.reserve(bytes);
}

// what the four inflate entry points ask of their arguments, device or host memory alike
static bool inflate_args_ok(const void *comp, size_t n_comp, const void *table, size_t n_blocks, const void *out, size_t n_out, const void *report)
{
    return report != nullptr && n_blocks < (size_t)0x7fffffff && n_comp < ((size_t)1 << 62) && n_out < ((size_t)1 << 62) &&
           (n_blocks == 0 || table != nullptr) && (n_comp == 0 || comp != nullptr) && (n_out == 0 || out != nullptr);
}

template <class F>
static int inflate_on_device(rocco_hip_solver *solver, const uint8_t *comp_dev, size_t n_comp, const int64_t *table_dev, size_t n_blocks,
                             uint8_t *out_dev, size_t n_out, int32_t *status_out_dev, int64_t *produced_out_dev, int64_t *report_out_host,
                             void *stream)
{
    if (solver == nullptr || !inflate_args_ok(comp_dev, n_comp, table_dev, n_blocks, out_dev, n_out, report_out_host)) {
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, inflate_scratch_bytes<F>(n_blocks)); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_inflate<F>(comp_dev, n_comp, table_dev, n_blocks, out_dev, n_out, status_out_dev, produced_out_dev, report_out_host,
                             solver->dev_misc.ptr, (hipStream_t)stream);
}

template <class F>
static int inflate_on_host(const uint8_t *comp, size_t n_comp, const int64_t *table, size_t n_blocks, uint8_t *out, size_t n_out,
                           int32_t *status_out, int64_t *produced_out, int64_t *report_out)
{
    if (!inflate_args_ok(comp, n_comp, table, n_blocks, out, n_out, report_out)) {
        return ROCCO_HIP_EINVAL;
    }
    inflate_host<F>(comp, (long long)n_comp, table, (long long)n_blocks, out, (long long)n_out, status_out, produced_out, report_out);
    return ROCCO_HIP_OK;
}

extern "C" {

int rocco_hip_abi_version(void) { return 1000; }

const char *rocco_hip_last_error(void) { return g_last_error.c_str(); }

int rocco_hip_solver_create(rocco_hip_solver **solver_out, int device)
{
    if (solver_out == nullptr) {
        return ROCCO_HIP_EINVAL;
    }
    *solver_out = nullptr;
    int count = 0;
    ROCCO_HIP_TRY(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) {
        set_last_error("rocco_hip_solver_create: no such HIP device");
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(device));
    rocco_hip_solver *s = new (std::nothrow) rocco_hip_solver();
    if (s == nullptr) {
        return ROCCO_HIP_ENOMEM;
    }
    s->device = device;
    *solver_out = s;
    return ROCCO_HIP_OK;
}

void rocco_hip_solver_destroy(rocco_hip_solver *solver)
{
    if (solver == nullptr) {
        return;
    }
    (void)hipSetDevice(solver->device);
    // whatever was queued with this handle's buffers has to be over before they go (a kernel that outlives its scratch
    // faults: "Memory access fault by GPU" at teardown)
    (void)hipDeviceSynchronize();
    solver->dev_tasks.release();
    solver->dev_params.release();
    solver->dev_results.release();
    solver->dev_bits.release();
    solver->dev_misc.release();
    solver->dev_select.release();
    solver->dev_solution.release();
    solver->dev_maps.release();
    solver->dev_frozen.release();
    solver->factor.reset();
    solver->dev_lean_pool.release();
    solver->dev_lean_round.release();
    solver->dev_lean_look.release();
    solver->dev_lean_desc.release();
    solver->dev_lean_wcap.release();
    solver->dev_chain.release();
    solver->host_chain.release();
    solver->host_follow.release();
    solver->host_objective.release();
    solver->dev_objective.release();
    solver->dev_map.release();
    solver->host_map_stage.release();
    solver->dev_median_partials.release();
    solver->host_lean_stage.release();
    solver->host_lean_back.release();
    solver->host_stage.release();
    solver->host_back.release();
    solver->host_table.release();
    delete solver;
}

int rocco_hip_solver_set(rocco_hip_solver *solver, const char *key, long long value)
{
    if (solver == nullptr || key == nullptr) {
        return ROCCO_HIP_EINVAL;
    }
    const std::string k(key);
    if (k == "force_exact") {
        solver->force_exact = value ? 1 : 0;
    } else if (k == "spec_depth") {
        if (value < 1 || value > 6) {
            return ROCCO_HIP_EINVAL;
        }
        solver->spec_depth = (int)value;
    } else if (k == "active_set") {
        solver->active_set = value ? 1 : 0;
    } else if (k == "lean") {
        solver->lean = value ? 1 : 0;
    } else if (k == "rolling_group_min") {
        if (value != 1 && value != 2 && value != 4 && value != 8) {
            return ROCCO_HIP_EINVAL;
        }
        solver->rolling_group_min = (int)value;
    } else {
        set_last_error("rocco_hip_solver_set: unknown key " + k);
        return ROCCO_HIP_EINVAL;
    }
    return ROCCO_HIP_OK;
}

int rocco_hip_score_median_batch(rocco_hip_solver *solver, const void *const *matrices_dev, int dtype, size_t K,
                                 const size_t *n, const size_t *row_strides, double *const *scores_dev, size_t count,
                                 void *stream)
{
    if (solver == nullptr || K == 0 || (dtype != 0 && dtype != 1) ||
        (count > 0 && (matrices_dev == nullptr || n == nullptr || row_strides == nullptr || scores_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    for (size_t i = 0; i < count; ++i) {
        if ((n[i] > 0 && (matrices_dev[i] == nullptr || scores_dev[i] == nullptr)) || row_strides[i] < n[i]) {
            return ROCCO_HIP_EINVAL;
        }
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_median_batch(matrices_dev, dtype, K, n, row_strides, scores_dev, count, (hipStream_t)stream);
}

int rocco_hip_score_median_batch_stats(rocco_hip_solver *solver, const void *const *matrices_dev, int dtype, size_t K,
                                       const size_t *n, const size_t *row_strides, double *const *scores_dev, size_t count,
                                       double *stats_dev, void *stream)
{
    if (stats_dev == nullptr) {
        return rocco_hip_score_median_batch(solver, matrices_dev, dtype, K, n, row_strides, scores_dev, count, stream);
    }
    if (solver == nullptr || K == 0 || (dtype != 0 && dtype != 1) ||
        (count > 0 && (matrices_dev == nullptr || n == nullptr || row_strides == nullptr || scores_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    for (size_t i = 0; i < count; ++i) {
        if (n[i] == 0 || matrices_dev[i] == nullptr || scores_dev[i] == nullptr || row_strides[i] < n[i]) {
            return ROCCO_HIP_EINVAL;  // (statistics of an empty score array do not exist)
        }
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    const size_t blocks = median_partials_count(n, count);
    int rc;
    if ((rc = solver->dev_median_partials.reserve(3 * blocks * sizeof(double) + 256)) != ROCCO_HIP_OK) return rc;
    return launch_median_batch(matrices_dev, dtype, K, n, row_strides, scores_dev, count, (hipStream_t)stream, stats_dev,
                               (double *)solver->dev_median_partials.ptr);
}

int rocco_hip_score_median(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K,
                           size_t n, size_t row_stride, double *scores_dev, void *stream)
{
    if (solver == nullptr || matrix_dev == nullptr || scores_dev == nullptr || K == 0 ||
        row_stride < n || (dtype != 0 && dtype != 1)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_median(matrix_dev, dtype, K, n, row_stride, scores_dev, (hipStream_t)stream);
}

int rocco_hip_score_order_statistic(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K, size_t n,
                                    size_t row_stride, int rank, double *scores_dev, void *stream)
{
    if (solver == nullptr || (n > 0 && (matrix_dev == nullptr || scores_dev == nullptr)) || K == 0 || row_stride < n ||
        (dtype != 0 && dtype != 1) || rank < 0 || (size_t)rank >= K) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_order_statistic(matrix_dev, dtype, K, n, row_stride, rank, scores_dev, (hipStream_t)stream);
}

int rocco_hip_score_trimmed_mean(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K, size_t n,
                                 size_t row_stride, int rank_lo, int rank_hi, double *scores_dev, void *stream)
{
    if (solver == nullptr || matrix_dev == nullptr || scores_dev == nullptr || K == 0 || row_stride < n ||
        (dtype != 0 && dtype != 1) || rank_lo < 0 || rank_hi < rank_lo || rank_hi >= (int)K) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_trimmed_mean(matrix_dev, dtype, K, n, row_stride, rank_lo, rank_hi, scores_dev, (hipStream_t)stream);
}

int rocco_hip_power_f64(rocco_hip_solver *solver, const double *x_dev, double power, double *out_dev, size_t n, void *stream)
{
    if (solver == nullptr || (n > 0 && (x_dev == nullptr || out_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_power(x_dev, power, out_dev, n, (hipStream_t)stream);
}

int rocco_hip_score_mean(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K, size_t n,
                         size_t row_stride, double *scores_dev, void *stream)
{
    if (solver == nullptr || (n > 0 && (matrix_dev == nullptr || scores_dev == nullptr)) || K == 0 || row_stride < n ||
        (dtype != 0 && dtype != 1)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_column_mean(matrix_dev, dtype, K, n, row_stride, scores_dev, (hipStream_t)stream);
}

// the checks the four dispersion entries share (K == 1 is answered by the caller without a launch: rocco/rocco.py:318-319)
static bool dispersion_args_ok(const rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride,
                               const double *scores_dev)
{
    return solver != nullptr && (n == 0 || (matrix_dev != nullptr && scores_dev != nullptr)) && K >= 2 && K <= 0x7FFFFFFF &&
           row_stride >= n && (dtype == 0 || dtype == 1);
}

int rocco_hip_score_mad(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride,
                        double *scores_dev, void *stream)
{
    if (!dispersion_args_ok(solver, matrix_dev, dtype, K, n, row_stride, scores_dev)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_mad(matrix_dev, dtype, K, n, row_stride, scores_dev, (hipStream_t)stream);
}

int rocco_hip_score_percentile_range(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K, size_t n,
                                     size_t row_stride, int index_lo, double g_lo, int index_hi, double g_hi,
                                     double *scores_dev, void *stream)
{
    if (!dispersion_args_ok(solver, matrix_dev, dtype, K, n, row_stride, scores_dev) || index_lo < 0 || index_hi < 0 ||
        (size_t)index_lo >= K || (size_t)index_hi >= K || !(g_lo >= 0.0 && g_lo < 1.0) || !(g_hi >= 0.0 && g_hi < 1.0)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_percentile_range(matrix_dev, dtype, K, n, row_stride, index_lo, g_lo, index_hi, g_hi, scores_dev,
                                   (hipStream_t)stream);
}

int rocco_hip_score_std(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K, size_t n, size_t row_stride,
                        int pairwise_order, double *scores_dev, void *stream)
{
    if (!dispersion_args_ok(solver, matrix_dev, dtype, K, n, row_stride, scores_dev)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_std(matrix_dev, dtype, K, n, row_stride, pairwise_order, scores_dev, (hipStream_t)stream);
}

int rocco_hip_score_trimmed_std(rocco_hip_solver *solver, const void *matrix_dev, int dtype, size_t K, size_t n,
                                size_t row_stride, int rank_lo, int rank_hi, int take_root, double *scores_dev, void *stream)
{
    if (!dispersion_args_ok(solver, matrix_dev, dtype, K, n, row_stride, scores_dev) || rank_lo < 0 || rank_hi < rank_lo ||
        (size_t)rank_hi >= K) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_trimmed_std(matrix_dev, dtype, K, n, row_stride, rank_lo, rank_hi, take_root, scores_dev, (hipStream_t)stream);
}

int rocco_hip_solve_penalized_chain_f64(rocco_hip_solver *solver, const double *scores_dev,
                                        const double *switch_costs_dev, double gamma, size_t n,
                                        double selection_penalty, uint8_t *solution_dev,
                                        double *value_out, long long *count_out, int *path_out,
                                        void *stream)
{
    if (solver == nullptr || scores_dev == nullptr || n == 0 || n >= ((size_t)1 << 31)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return solve_fixed_penalty(solver, scores_dev, switch_costs_dev, gamma, n, selection_penalty,
                               solution_dev, value_out, count_out, path_out, (hipStream_t)stream);
}

int rocco_hip_solve_budget_batch_f64(rocco_hip_solver *solver, size_t n_tasks,
                                     const rocco_hip_budget_task *tasks,
                                     rocco_hip_budget_result *results, void *stream)
{
    if (solver == nullptr || (n_tasks > 0 && (tasks == nullptr || results == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    for (size_t t = 0; t < n_tasks; ++t) {
        if (tasks[t].scores_dev == nullptr || tasks[t].n == 0 || tasks[t].n >= ((size_t)1 << 31) ||
            tasks[t].solution_dev == nullptr || tasks[t].max_iter < 0) {
            return ROCCO_HIP_EINVAL;
        }
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return solve_budget_batch(solver, n_tasks, tasks, results, (hipStream_t)stream);
}

int rocco_hip_solve_budget_batch_stats_f64(rocco_hip_solver *solver, size_t n_tasks, const rocco_hip_budget_task *tasks,
                                           const double *score_stats_host, rocco_hip_budget_result *results, void *stream)
{
    if (solver == nullptr || (n_tasks > 0 && (tasks == nullptr || results == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    for (size_t t = 0; t < n_tasks; ++t) {
        if (tasks[t].scores_dev == nullptr || tasks[t].n == 0 || tasks[t].n >= ((size_t)1 << 31) ||
            tasks[t].solution_dev == nullptr || tasks[t].max_iter < 0) {
            return ROCCO_HIP_EINVAL;
        }
        if (score_stats_host != nullptr && !(score_stats_host[3 * t] <= score_stats_host[3 * t + 1])) {
            return ROCCO_HIP_EINVAL;  // min <= max (also refuses NaN)
        }
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return solve_budget_batch(solver, n_tasks, tasks, results, (hipStream_t)stream, score_stats_host);
}

int rocco_hip_delta_model_lean_f64(rocco_hip_solver *solver, const double *scores_dev, double gamma, size_t n,
                                   const uint8_t *emap_dev, const double *lambdas, size_t n_lambdas, long long *counts_out,
                                   long long *open_out, void *stream)
{
    if (solver == nullptr || scores_dev == nullptr || emap_dev == nullptr || n < 2 || n >= ((size_t)1 << 31) ||
        (n_lambdas > 0 && (lambdas == nullptr || counts_out == nullptr || open_out == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return delta_model_lean(solver, scores_dev, gamma, n, emap_dev, lambdas, n_lambdas, counts_out, open_out, (hipStream_t)stream);
}

int rocco_hip_delta_probe_f64(rocco_hip_solver *solver, const double *scores_dev,
                              const double *switch_costs_dev, double gamma, size_t n,
                              const uint8_t *emap_dev, const double *lambdas, size_t n_lambdas,
                              rocco_hip_probe_stats *stats_out, void *stream)
{
    if (solver == nullptr || scores_dev == nullptr || n == 0 || n >= ((size_t)1 << 31) ||
        (n_lambdas > 0 && (lambdas == nullptr || stats_out == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return delta_probe(solver, scores_dev, switch_costs_dev, gamma, n, emap_dev, lambdas, n_lambdas,
                       stats_out, (hipStream_t)stream);
}

int rocco_hip_delta_bound_rounds_f64(rocco_hip_solver *solver, const double *scores_dev, double gamma, size_t n,
                                     const double *lambdas, const int *round_sizes, int n_rounds,
                                     double *lambdas_used_out, long long *counts_out, long long *level_len_out,
                                     void *stream)
{
    if (solver == nullptr || scores_dev == nullptr || n < 2 || n >= ((size_t)1 << 31) || n_rounds < 0 ||
        (n_rounds > 0 && (lambdas == nullptr || round_sizes == nullptr || lambdas_used_out == nullptr ||
                          counts_out == nullptr || level_len_out == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return delta_bound_rounds(solver, scores_dev, gamma, n, lambdas, round_sizes, n_rounds, lambdas_used_out, counts_out,
                              level_len_out, (hipStream_t)stream);
}

int rocco_hip_delta_spine_f64(rocco_hip_solver *solver, const double *scores_dev,
                              const double *switch_costs_dev, double gamma, size_t n,
                              const uint8_t *emap_dev, const double *lambdas, size_t n_lambdas,
                              int solution_index, uint8_t *solution_dev, long long *counts_out,
                              void *stream)
{
    if (solver == nullptr || scores_dev == nullptr || n == 0 || n >= ((size_t)1 << 31) || emap_dev == nullptr ||
        lambdas == nullptr || counts_out == nullptr || n_lambdas == 0 || n_lambdas > 64 ||
        solution_index >= (int)n_lambdas || (solution_index >= 0 && solution_dev == nullptr)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return delta_spine(solver, scores_dev, switch_costs_dev, gamma, n, emap_dev, lambdas, n_lambdas,
                       solution_index, solution_dev, counts_out, (hipStream_t)stream);
}

int rocco_hip_delta_build_map_f64(rocco_hip_solver *solver, const double *scores_dev,
                                  const double *switch_costs_dev, double gamma, size_t n,
                                  double lambda_ref, double margin, uint8_t *emap_dev, void *stream)
{
    if (solver == nullptr || scores_dev == nullptr || n == 0 || n >= ((size_t)1 << 31) || emap_dev == nullptr ||
        !(margin >= 0.0)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return delta_build_map(solver, scores_dev, switch_costs_dev, gamma, n, lambda_ref, margin, emap_dev,
                           (hipStream_t)stream);
}

int rocco_hip_delta_build_map_lean_f64(rocco_hip_solver *solver, const double *scores_dev, double gamma, size_t n,
                                       double lambda_ref, double margin, uint8_t *emap_dev, void *stream)
{
    if (solver == nullptr || scores_dev == nullptr || n < 2 || n >= ((size_t)1 << 31) || emap_dev == nullptr || !(margin >= 0.0)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return delta_build_map_lean(solver, scores_dev, gamma, n, lambda_ref, margin, emap_dev, (hipStream_t)stream);
}

int rocco_hip_delta_window_f64(rocco_hip_solver *solver, const double *scores_dev,
                               const double *switch_costs_dev, double gamma, size_t n,
                               const uint8_t *emap_dev, double lambda_lo, double lambda_hi,
                               uint8_t *solution_dev, rocco_hip_window_stats *stats_out, void *stream)
{
    if (solver == nullptr || scores_dev == nullptr || n == 0 || n >= ((size_t)1 << 31) ||
        solution_dev == nullptr || stats_out == nullptr || !(lambda_lo <= lambda_hi)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return delta_window(solver, scores_dev, switch_costs_dev, gamma, n, emap_dev, lambda_lo, lambda_hi,
                        solution_dev, stats_out, (hipStream_t)stream);
}

int rocco_hip_objective_value_f64(rocco_hip_solver *solver, const uint8_t *solution_dev,
                                  const double *scores_dev, const double *switch_costs_dev,
                                  double gamma, size_t n, double *objective_out, void *stream)
{
    if (solver == nullptr || objective_out == nullptr || (n > 0 && (solution_dev == nullptr || scores_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    int rc = solver->dev_misc.reserve(objective_scratch_bytes(n));
    if (rc != ROCCO_HIP_OK) {
        return rc;
    }
    rc = solver->host_back.reserve(64);
    if (rc != ROCCO_HIP_OK) {
        return rc;
    }
    double *back = (double *)solver->host_back.ptr;
    rc = launch_objective(solution_dev, scores_dev, switch_costs_dev, gamma, n, solver->dev_misc.ptr,
                          back, (hipStream_t)stream);
    if (rc == ROCCO_HIP_OK) {
        *objective_out = *back;
    }
    return rc;
}

int rocco_hip_peak_signal_stat_f64(rocco_hip_solver *solver, const double *counts_dev, const double *lengths_dev, size_t n_peaks,
                                   size_t n_samples, double row_scale, double pc, double percentile, double *stat_out_dev, void *stream)
{
    if (solver == nullptr || n_samples == 0 || n_samples > 4096 || !(percentile >= 0.0 && percentile <= 100.0) ||
        (n_peaks > 0 && (counts_dev == nullptr || lengths_dev == nullptr || stat_out_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    const int rc = solver->dev_misc.reserve(n_peaks * n_samples * sizeof(double) + 256);
    if (rc != ROCCO_HIP_OK) return rc;
    return launch_peak_signal(counts_dev, lengths_dev, n_peaks, n_samples, row_scale, pc, percentile, stat_out_dev, solver->dev_misc.ptr,
                              (hipStream_t)stream);
}

int rocco_hip_ecdf_survival_f64(rocco_hip_solver *solver, const double *stat_dev, const int *bin_dev, const double *null_values_dev,
                                const long long *null_offsets_dev, size_t n_peaks, double *pvals_out_dev, void *stream)
{
    if (solver == nullptr || (n_peaks > 0 && (stat_dev == nullptr || bin_dev == nullptr || null_values_dev == nullptr ||
                                              null_offsets_dev == nullptr || pvals_out_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_ecdf_survival(stat_dev, bin_dev, null_values_dev, null_offsets_dev, n_peaks, pvals_out_dev, (hipStream_t)stream);
}

int rocco_hip_bh_adjust_f64(rocco_hip_solver *solver, const double *pvals_dev, size_t m, double *qvals_out_dev, void *stream)
{
    if (solver == nullptr || m >= ((size_t)1 << 31) || (m > 0 && (pvals_dev == nullptr || qvals_out_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    const int rc = solver->dev_misc.reserve(bh_scratch_bytes(m));
    if (rc != ROCCO_HIP_OK) return rc;
    return launch_bh_adjust(pvals_dev, m, qvals_out_dev, solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_sort_f64(rocco_hip_solver *solver, const double *x_dev, size_t n, double *sorted_out_dev, void *stream)
{
    if (solver == nullptr || (n > 0 && (x_dev == nullptr || sorted_out_dev == nullptr)) || n >= ((size_t)1 << 31)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    const int rc = solver->dev_misc.reserve(sort_f64_scratch_bytes(n));
    if (rc != ROCCO_HIP_OK) return rc;
    return launch_sort_f64(x_dev, n, sorted_out_dev, solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_sorted_probe_f64(rocco_hip_solver *solver, const double *sorted_dev, size_t n, const long long *ranks,
                               size_t n_ranks, double *values_out, double shift, const double *thresholds,
                               size_t n_thresholds, long long *counts_le_out, long long *counts_lt_out, void *stream)
{
    if (solver == nullptr || sorted_dev == nullptr || n == 0 || n_ranks > 8 || n_thresholds > 8 ||
        (n_ranks > 0 && (ranks == nullptr || values_out == nullptr)) ||
        (n_thresholds > 0 && (thresholds == nullptr || counts_le_out == nullptr || counts_lt_out == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    SortedProbe p;
    p.n_ranks = (int)n_ranks;
    p.n_thresholds = (int)n_thresholds;
    p.shift = shift;
    for (size_t i = 0; i < 8; ++i) {
        p.ranks[i] = (i < n_ranks) ? ranks[i] : 0;
        p.thresholds[i] = (i < n_thresholds) ? thresholds[i] : 0.0;
    }
    int rc = solver->dev_results.reserve(8 * sizeof(double) + 16 * sizeof(long long) + 64);
    if (rc != ROCCO_HIP_OK) return rc;
    rc = solver->host_back.reserve(8 * sizeof(double) + 16 * sizeof(long long) + 64);
    if (rc != ROCCO_HIP_OK) return rc;
    double *d_vals = (double *)solver->dev_results.ptr;
    long long *d_cnts = (long long *)((char *)solver->dev_results.ptr + 64);
    rc = launch_sorted_probe(sorted_dev, n, p, d_vals, d_cnts, (hipStream_t)stream);
    if (rc != ROCCO_HIP_OK) return rc;
    ROCCO_HIP_TRY(hipMemcpyAsync(solver->host_back.ptr, solver->dev_results.ptr, 64 + 16 * sizeof(long long), hipMemcpyDeviceToHost,
                                 (hipStream_t)stream));
    ROCCO_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    const double *hv = (const double *)solver->host_back.ptr;
    const long long *hc = (const long long *)((const char *)solver->host_back.ptr + 64);
    for (size_t i = 0; i < n_ranks; ++i) values_out[i] = hv[i];
    for (size_t i = 0; i < n_thresholds; ++i) {
        counts_le_out[i] = hc[2 * i];
        counts_lt_out[i] = hc[2 * i + 1];
    }
    return ROCCO_HIP_OK;
}

int rocco_hip_select_ranks_batch_f64(rocco_hip_solver *solver, size_t count, const double *const *vectors_dev, const size_t *n,
                                     size_t n_ranks, const long long *ranks, int mode, const double *centers,
                                     double *values_out_dev, long long *counts_out_dev, void *stream)
{
    if (solver == nullptr || n_ranks > (size_t)kSelectRanksMax || (mode != 0 && mode != 1) ||
        (count > 0 && (vectors_dev == nullptr || n == nullptr || counts_out_dev == nullptr)) ||
        (count > 0 && n_ranks > 0 && (ranks == nullptr || values_out_dev == nullptr)) || (count > 0 && mode == 1 && centers == nullptr)) {
        return ROCCO_HIP_EINVAL;
    }
    for (size_t v = 0; v < count; ++v) {
        if (n[v] >= ((size_t)1 << 31) || (n[v] > 0 && vectors_dev[v] == nullptr) || (n[v] == 0 && n_ranks > 0)) {
            return ROCCO_HIP_EINVAL;
        }
        for (size_t r = 0; r < n_ranks; ++r) {
            if (ranks[v * n_ranks + r] < 0 || ranks[v * n_ranks + r] >= (long long)n[v]) {
                return ROCCO_HIP_EINVAL;
            }
        }
    }
    if (count == 0) {
        return ROCCO_HIP_OK;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    const int rc = solver->dev_select.reserve(select_scratch_bytes(count));
    if (rc != ROCCO_HIP_OK) return rc;
    return launch_select_ranks_batch(vectors_dev, n, count, (int)n_ranks, ranks, mode, centers, values_out_dev, counts_out_dev,
                                     solver->dev_select.ptr, (hipStream_t)stream);
}

int rocco_hip_bh_last_passing_rank_f64(rocco_hip_solver *solver, const double *sorted_dev, size_t m, double fdr,
                                       long long *rank_out_dev, void *stream)
{
    if (solver == nullptr || rank_out_dev == nullptr || (m > 0 && sorted_dev == nullptr) || m >= ((size_t)1 << 31)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_bh_last_passing_rank(sorted_dev, m, fdr, rank_out_dev, (hipStream_t)stream);
}

int rocco_hip_threshold_mask_f64(rocco_hip_solver *solver, const double *x_dev, size_t n, double divisor, double threshold,
                                 double floor_value, int use_floor, uint8_t *mask_out_dev, void *stream)
{
    if (solver == nullptr || (n > 0 && (x_dev == nullptr || mask_out_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_threshold_mask(x_dev, n, divisor, threshold, floor_value, use_floor, mask_out_dev, (hipStream_t)stream);
}

int rocco_hip_at_most_mask_f64(rocco_hip_solver *solver, const double *x_dev, size_t n, double cutoff, uint8_t *mask_out_dev,
                               void *stream)
{
    if (solver == nullptr || (n > 0 && (x_dev == nullptr || mask_out_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_at_most_mask(x_dev, n, cutoff, mask_out_dev, (hipStream_t)stream);
}

int rocco_hip_divide_finite_f64(rocco_hip_solver *solver, const double *x_dev, size_t n, double divisor, double *out_dev,
                                void *stream)
{
    if (solver == nullptr || (n > 0 && (x_dev == nullptr || out_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_divide_finite(x_dev, n, divisor, out_dev, (hipStream_t)stream);
}

int rocco_hip_autocovariance_sums_f64(rocco_hip_solver *solver, const double *x_dev, size_t n, double mean, int max_lag,
                                      double *sums_out, void *stream)
{
    if (solver == nullptr || x_dev == nullptr || n == 0 || sums_out == nullptr || max_lag < 0 || (size_t)max_lag >= n) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    int rc = solver->dev_misc.reserve(autocov_scratch_bytes(n, max_lag));
    if (rc != ROCCO_HIP_OK) return rc;
    rc = solver->dev_results.reserve(((size_t)max_lag + 1024) * sizeof(double));
    if (rc != ROCCO_HIP_OK) return rc;
    rc = solver->host_back.reserve(((size_t)max_lag + 1024) * sizeof(double));
    if (rc != ROCCO_HIP_OK) return rc;
    rc = launch_autocov(x_dev, n, mean, max_lag, (double *)solver->dev_results.ptr, solver->dev_misc.ptr, (hipStream_t)stream);
    if (rc != ROCCO_HIP_OK) return rc;
    ROCCO_HIP_TRY(hipMemcpyAsync(solver->host_back.ptr, solver->dev_results.ptr, (size_t)(max_lag + 1) * sizeof(double),
                                 hipMemcpyDeviceToHost, (hipStream_t)stream));
    ROCCO_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    std::memcpy(sums_out, solver->host_back.ptr, (size_t)(max_lag + 1) * sizeof(double));
    return ROCCO_HIP_OK;
}

int rocco_hip_negative_part_f64(rocco_hip_solver *solver, const double *scores_dev, double *out_dev, size_t n, void *stream)
{
    if (solver == nullptr || (n > 0 && (scores_dev == nullptr || out_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_negative_part(scores_dev, out_dev, n, (hipStream_t)stream);
}

int rocco_hip_soft_counts_f64(rocco_hip_solver *solver, const double *scores_dev, double center, double scale, double *out_dev,
                              size_t n, void *stream)
{
    if (solver == nullptr || (n > 0 && (scores_dev == nullptr || out_dev == nullptr)) || !(scale > 0.0)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_soft_counts(scores_dev, center, scale, out_dev, n, (hipStream_t)stream);
}

int rocco_hip_decode_runs_batch(rocco_hip_solver *solver, size_t count, const uint8_t *const *solutions_dev, const size_t *n,
                                int64_t *const *run_begin_dev, int64_t *const *run_end_dev, const size_t *capacities,
                                size_t *n_runs_out, void *stream)
{
    if (solver == nullptr || (count > 0 && (solutions_dev == nullptr || n == nullptr || run_begin_dev == nullptr ||
                                            run_end_dev == nullptr || capacities == nullptr || n_runs_out == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    size_t at = 0;
    while (at < count) {
        DecodeBatch batch;
        batch.n_tasks = 0;
        batch.pad = 0;
        long long tiles = 0;
        size_t owner[kDecodeBatchMax];
        while (at < count && batch.n_tasks < kDecodeBatchMax) {
            n_runs_out[at] = 0;
            if (n[at] > 1) {
                if (solutions_dev[at] == nullptr || (capacities[at] > 0 && (run_begin_dev[at] == nullptr || run_end_dev[at] == nullptr))) {
                    return ROCCO_HIP_EINVAL;
                }
                DecodeTask &t = batch.tasks[batch.n_tasks];
                t.solution = solutions_dev[at];
                t.n = (long long)n[at];
                t.tile_begin = tiles;
                t.run_begin = run_begin_dev[at];
                t.run_end = run_end_dev[at];
                t.capacity = (unsigned long long)capacities[at];
                owner[batch.n_tasks++] = at;
                tiles += decode_tiles(n[at]);
            }
            ++at;
        }
        if (batch.n_tasks == 0) {
            continue;
        }
        int rc = solver->dev_misc.reserve(decode_batch_scratch_bytes(tiles, batch.n_tasks));
        if (rc != ROCCO_HIP_OK) return rc;
        rc = solver->host_back.reserve((size_t)batch.n_tasks * 16 + 64);
        if (rc != ROCCO_HIP_OK) return rc;
        unsigned long long *back = (unsigned long long *)solver->host_back.ptr;
        rc = launch_decode_runs_batch(batch, tiles, solver->dev_misc.ptr, back, (hipStream_t)stream);
        if (rc != ROCCO_HIP_OK) return rc;
        for (int i = 0; i < batch.n_tasks; ++i) {
            n_runs_out[owner[i]] = (size_t)back[2 * i];
        }
    }
    return ROCCO_HIP_OK;
}

int rocco_hip_decode_runs_table(rocco_hip_solver *solver, size_t count, const uint8_t *const *solutions_dev, const size_t *n,
                                const long long *units, int64_t *table_dev, size_t capacity_rows, size_t eager_rows,
                                size_t *row_offsets_out, const int64_t **table_host_out, void *stream)
{
    if (solver == nullptr || row_offsets_out == nullptr || count > (size_t)kDecodeBatchMax ||
        (count > 0 && (solutions_dev == nullptr || n == nullptr || units == nullptr)) || (capacity_rows > 0 && table_dev == nullptr)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    if (table_host_out != nullptr) {
        *table_host_out = nullptr;
    }
    DecodeBatch batch;
    batch.n_tasks = 0;
    batch.pad = 0;
    long long tiles = 0;
    size_t owner[kDecodeBatchMax];
    for (size_t at = 0; at < count; ++at) {
        row_offsets_out[at] = 0;
        if (n[at] > 1) {
            if (solutions_dev[at] == nullptr) {
                return ROCCO_HIP_EINVAL;
            }
            DecodeTask &t = batch.tasks[batch.n_tasks];
            t.solution = solutions_dev[at];
            t.n = (long long)n[at];
            t.tile_begin = tiles;
            t.run_begin = table_dev;
            t.run_end = nullptr;
            t.capacity = (unsigned long long)capacity_rows;
            t.unit = units[at];
            owner[batch.n_tasks++] = at;
            tiles += decode_tiles(n[at]);
        }
    }
    row_offsets_out[count] = 0;
    if (batch.n_tasks == 0) {
        return ROCCO_HIP_OK;
    }
    int rc = solver->dev_misc.reserve(decode_batch_scratch_bytes(tiles, batch.n_tasks));
    if (rc != ROCCO_HIP_OK) return rc;
    rc = solver->host_back.reserve((size_t)batch.n_tasks * 16 + 64);
    if (rc != ROCCO_HIP_OK) return rc;
    const bool want_host = (table_host_out != nullptr);
    (void)eager_rows;  // (was: how many rows to copy before their number is known; the rows that exist are copied by a kernel now)
    const size_t eager = want_host ? capacity_rows : 0;
    if (want_host) {
        rc = solver->host_table.reserve(std::max<size_t>(capacity_rows, 1) * 3 * sizeof(int64_t));
        if (rc != ROCCO_HIP_OK) return rc;
    }
    unsigned long long *back = (unsigned long long *)solver->host_back.ptr;
    int64_t *host_rows = want_host ? (int64_t *)solver->host_table.ptr : nullptr;
    rc = launch_decode_runs_table(batch, tiles, solver->dev_misc.ptr, table_dev, back, host_rows, eager, (hipStream_t)stream);
    if (rc != ROCCO_HIP_OK) return rc;
    // per-solution row ranges: row_offsets_out[i] .. row_offsets_out[i + 1]
    size_t total = 0;
    int next = 0;
    for (size_t at = 0; at < count; ++at) {
        row_offsets_out[at] = total;
        if (next < batch.n_tasks && owner[next] == at) {
            total += (size_t)back[2 * next];
            ++next;
        }
    }
    row_offsets_out[count] = total;
    if (want_host && total <= capacity_rows) {
        if (total > eager) {  // the eager copy did not cover the table: the rest, and one more synchronisation
            ROCCO_HIP_TRY(hipMemcpyAsync(host_rows + 3 * eager, table_dev + 3 * eager, (total - eager) * 3 * sizeof(int64_t),
                                         hipMemcpyDeviceToHost, (hipStream_t)stream));
            ROCCO_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        }
        *table_host_out = host_rows;
    }
    return ROCCO_HIP_OK;
}

int rocco_hip_decode_runs(rocco_hip_solver *solver, const uint8_t *solution_dev, size_t n,
                          int64_t *run_begin_dev, int64_t *run_end_dev, size_t capacity,
                          size_t *n_runs_out, void *stream)
{
    if (solver == nullptr || n_runs_out == nullptr || (n > 0 && solution_dev == nullptr) ||
        (capacity > 0 && (run_begin_dev == nullptr || run_end_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    int rc = solver->dev_misc.reserve(decode_scratch_bytes(n));
    if (rc != ROCCO_HIP_OK) {
        return rc;
    }
    rc = solver->host_back.reserve(64);
    if (rc != ROCCO_HIP_OK) {
        return rc;
    }
    unsigned long long *back = (unsigned long long *)solver->host_back.ptr;
    rc = launch_decode_runs(solution_dev, n, run_begin_dev, run_end_dev, capacity, solver->dev_misc.ptr,
                            back, (hipStream_t)stream);
    if (rc == ROCCO_HIP_OK) {
        *n_runs_out = (size_t)*back;
    }
    return rc;
}

namespace {

// The LDL^T factor depends on the penalty and (at its last two entries only) on the length: the solver keeps the one of
// the longest row seen with this penalty.  The recurrence is sequential and data-independent: two host threads walk it
// (whittaker_host.cpp, ~10 ns per step against ~190 ns for a GPU lane: 0.1 s instead of 1.05 s for chr1 at 50 bp) and the
// table is copied up.  A longer row with the same penalty extends the factor instead of starting over; a new penalty
// starts a new one.
std::mutex g_factor_mutex;
// per device; on the heap and never destroyed: at process exit the HIP runtime may be gone before static destructors run
// per (device, penalty): a batch that mixes short contigs (a window below 101 loci: another penalty) with chromosomes keeps both
std::map<std::pair<int, double>, std::shared_ptr<rocco::SharedFactor>> &g_factors = *new std::map<std::pair<int, double>, std::shared_ptr<rocco::SharedFactor>>();

// the device's factor covers `cols` loci at this penalty when this returns; solver->factor holds it for the call
int ensure_whittaker_factor(rocco_hip_solver *solver, size_t cols, double penalty_lambda, hipStream_t stream)
{
    if (cols < 25) {
        return ROCCO_HIP_OK;
    }
    std::lock_guard<std::mutex> lock(g_factor_mutex);  // (a second thread waits for the first one's factor rather than building its own)
    std::shared_ptr<rocco::SharedFactor> &current = g_factors[std::make_pair(solver->device, penalty_lambda)];
    if (current && current->cap >= cols && current->lambda == penalty_lambda) {
        solver->factor = current;
        return ROCCO_HIP_OK;
    }
    auto grown = std::make_shared<rocco::SharedFactor>();
    grown->device = solver->device;
    int rc;
    if ((rc = grown->buf.reserve(6 * cols * sizeof(double))) != ROCCO_HIP_OK) {
        return rc;
    }
    const bool extend = current && current->cap > 0 && current->lambda == penalty_lambda;
    // (ROCCO_HIP_FACTOR_ON_DEVICE=1: the recurrence walked by one GPU lane per parity instead of two host threads)
    const char *on_device = std::getenv("ROCCO_HIP_FACTOR_ON_DEVICE");
    rc = (on_device != nullptr && std::atoi(on_device) != 0)
             ? launch_whittaker_factor(cols, penalty_lambda, (double *)grown->buf.ptr, stream,
                                       extend ? (const double *)current->buf.ptr : nullptr, extend ? current->cap : 0)
             : build_whittaker_factor_on_host(cols, penalty_lambda, (double *)grown->buf.ptr, stream,
                                              extend ? (const double *)current->buf.ptr : nullptr, extend ? current->cap : 0);
    if (rc == ROCCO_HIP_OK && hipStreamSynchronize(stream) != hipSuccess) {
        rc = ROCCO_HIP_EHIP;
    }
    if (rc != ROCCO_HIP_OK) {
        return rc;
    }
    grown->cap = cols;
    grown->lambda = penalty_lambda;
    current = grown;
    solver->factor = grown;
    return ROCCO_HIP_OK;
}

}  // namespace

namespace {

int whittaker_batch(rocco_hip_solver *solver, size_t count, const double *const *matrices_dev, const double *const *offsets_dev,
                    const size_t *rows, const size_t *cols, double penalty_lambda, double *const *baselines_dev, int residual,
                    void *stream, void *scratch_dev = nullptr, size_t scratch_bytes = 0)
{
    if (solver == nullptr || (count > 0 && (matrices_dev == nullptr || rows == nullptr || cols == nullptr || baselines_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    size_t longest = 0;
    for (size_t i = 0; i < count; ++i) {
        if (rows[i] * cols[i] > 0 && (matrices_dev[i] == nullptr || baselines_dev[i] == nullptr || (residual != 0 && baselines_dev[i] == matrices_dev[i]))) {
            return ROCCO_HIP_EINVAL;
        }
        if (rows[i] > 0) {
            longest = std::max(longest, cols[i]);
        }
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    int rc;
    if (scratch_dev != nullptr) {  // (the caller's block: what the sweeps need between them, see rocco_hip_whittaker_batch_scratch_bytes)
        if (scratch_bytes < whittaker_batch_scratch_bytes(rows, cols, count) || ((uintptr_t)scratch_dev & 255u) != 0) {
            set_last_error("the sweeps' scratch block is too small or not aligned to 256 bytes");
            return ROCCO_HIP_EINVAL;
        }
    } else if ((rc = solver->dev_misc.reserve(whittaker_batch_scratch_bytes(rows, cols, count))) != ROCCO_HIP_OK) {
        return rc;
    }
    if ((rc = solver->host_stage.reserve(whittaker_batch_stage_bytes(rows, cols, count))) != ROCCO_HIP_OK) return rc;
    if ((rc = ensure_whittaker_factor(solver, longest, penalty_lambda, (hipStream_t)stream)) != ROCCO_HIP_OK) return rc;
    const rocco::SharedFactor *factor = (longest >= 25) ? solver->factor.get() : nullptr;
    rc = launch_crossfit_whittaker_batch(matrices_dev, rows, cols, count, penalty_lambda,
                                         factor != nullptr ? (const double *)factor->buf.ptr : nullptr,
                                         factor != nullptr ? factor->cap : 0, baselines_dev,
                                         scratch_dev != nullptr ? scratch_dev : solver->dev_misc.ptr,
                                         solver->host_stage.ptr, (hipStream_t)stream, offsets_dev, residual);
    if (rc != ROCCO_HIP_OK) {
        return rc;
    }
    ROCCO_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the scratch buffers are the solver's
    if (whittaker_collect_repairs(solver->host_stage.ptr) != 0 && residual != 0) {
        set_last_error("Local baseline fit produced non-finite values");
        return ROCCO_HIP_EINVAL;
    }
    return ROCCO_HIP_OK;
}

}  // namespace

int rocco_hip_crossfit_whittaker_baseline_batch_f64(rocco_hip_solver *solver, size_t count, const double *const *matrices_dev,
                                                    const size_t *rows, const size_t *cols, double penalty_lambda,
                                                    double *const *baselines_dev, void *stream)
{
    return whittaker_batch(solver, count, matrices_dev, nullptr, rows, cols, penalty_lambda, baselines_dev, 0, stream);
}

int rocco_hip_crossfit_whittaker_residual_batch_f64(rocco_hip_solver *solver, size_t count, const double *const *matrices_dev,
                                                    const double *const *row_offsets_dev, const size_t *rows, const size_t *cols,
                                                    double penalty_lambda, double *const *centered_out_dev, void *stream)
{
    return whittaker_batch(solver, count, matrices_dev, row_offsets_dev, rows, cols, penalty_lambda, centered_out_dev, 1, stream);
}

size_t rocco_hip_whittaker_batch_scratch_bytes(size_t count, const size_t *rows, const size_t *cols)
{
    return (rows == nullptr || cols == nullptr) ? 0 : whittaker_batch_scratch_bytes(rows, cols, count);
}

int rocco_hip_crossfit_whittaker_residual_batch_scratch_f64(rocco_hip_solver *solver, size_t count, const double *const *matrices_dev,
                                                            const double *const *row_offsets_dev, const size_t *rows,
                                                            const size_t *cols, double penalty_lambda, double *const *centered_out_dev,
                                                            void *scratch_dev, size_t scratch_bytes, void *stream)
{
    if (scratch_dev == nullptr) {
        return ROCCO_HIP_EINVAL;
    }
    return whittaker_batch(solver, count, matrices_dev, row_offsets_dev, rows, cols, penalty_lambda, centered_out_dev, 1, stream,
                           scratch_dev, scratch_bytes);
}

int rocco_hip_crossfit_whittaker_baseline_matrix_f64(rocco_hip_solver *solver, const double *matrix_dev,
                                                     size_t rows, size_t cols, double penalty_lambda,
                                                     double *baseline_out_dev, void *stream)
{
    if (solver == nullptr || ((matrix_dev == nullptr || baseline_out_dev == nullptr) && rows * cols > 0)) {
        return ROCCO_HIP_EINVAL;
    }
    return rocco_hip_crossfit_whittaker_baseline_batch_f64(solver, 1, &matrix_dev, &rows, &cols, penalty_lambda, &baseline_out_dev,
                                                           stream);
}

int rocco_hip_wls_rolling_variances_batch_f64(rocco_hip_solver *solver, size_t count, const double *const *centered_dev,
                                              const size_t *K, const size_t *n, int spatial_window, double *const *variances_dev,
                                              void *stream)
{
    if (solver == nullptr || (count > 0 && (centered_dev == nullptr || K == nullptr || n == nullptr || variances_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    size_t rows = 0;
    for (size_t i = 0; i < count; ++i) {
        const int window = wls_spatial_window(n[i], spatial_window);
        if (window > wls_max_window()) {
            set_last_error("rocco_hip_wls_rolling_variances_batch_f64: spatial windows above 63 loci go through the single-matrix call");
            return ROCCO_HIP_EINVAL;
        }
        if (window > 0 && n[i] >= 4) {
            if (centered_dev[i] == nullptr || variances_dev[i] == nullptr) {
                return ROCCO_HIP_EINVAL;
            }
            rows += K[i];
        }
    }
    if (rows == 0) {
        return ROCCO_HIP_OK;
    }
    // rows per workgroup (one task record each); a solver may ask for at least so many (rocco_hip_solver_set "rolling_group_min")
    wls_set_rolling_group_min(solver->rolling_group_min);
    const size_t group = (size_t)wls_rolling_group_rows(rows);
    int rc;
    if ((rc = solver->dev_tasks.reserve(rows * sizeof(WlsRollingTask))) != ROCCO_HIP_OK) return rc;
    if ((rc = solver->host_stage.reserve(rows * sizeof(WlsRollingTask))) != ROCCO_HIP_OK) return rc;
    WlsRollingTask *host = (WlsRollingTask *)solver->host_stage.ptr;
    size_t t = 0;
    for (size_t i = 0; i < count; ++i) {
        const int window = wls_spatial_window(n[i], spatial_window);
        if (window <= 0 || n[i] < 4) {
            continue;
        }
        const size_t stride = n[i] - (size_t)window + 1;
        for (size_t k = 0; k < K[i]; k += group, ++t) {
            host[t].row = centered_dev[i] + k * n[i];
            host[t].n = (long long)n[i];
            host[t].window = window;
            host[t].rows = (int)std::min(group, K[i] - k);
            host[t].out = variances_dev[i] + k * stride;
        }
    }
    ROCCO_HIP_TRY(hipMemcpyAsync(solver->dev_tasks.ptr, host, t * sizeof(WlsRollingTask), hipMemcpyHostToDevice, (hipStream_t)stream));
    if ((rc = launch_wls_rolling_batch((const WlsRollingTask *)solver->dev_tasks.ptr, t, (int)group, (hipStream_t)stream)) != ROCCO_HIP_OK) return rc;
    ROCCO_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the task table is the solver's
    return ROCCO_HIP_OK;
}

long long rocco_hip_buffer_growths(void) { return g_buffer_growths.load(std::memory_order_relaxed); }

long long rocco_hip_whittaker_seam_repairs(void) { return whittaker_seam_repairs(); }

int rocco_hip_whittaker_batch_plan(rocco_hip_solver *solver, size_t count, const size_t *rows, const size_t *cols, int residual,
                                   int with_offsets, int *n_seg_out, long long *seg_tiles_out, long long *info_out)
{
    if (solver == nullptr || info_out == nullptr || (count > 0 && (rows == nullptr || cols == nullptr || n_seg_out == nullptr || seg_tiles_out == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device));
    return whittaker_batch_plan(rows, cols, count, residual, with_offsets, n_seg_out, seg_tiles_out, info_out);
}

void rocco_hip_model_chain_counters(long long out[4])
{
    if (out != nullptr) {
        rocco::model_chain_counters(out);
    }
}

void rocco_hip_model_chain_written_counters(long long out[2])
{
    if (out != nullptr) {
        rocco::model_chain_written_counters(out);
    }
}

long long rocco_hip_solver_device_bytes(const rocco_hip_solver *solver)
{
    if (solver == nullptr) {
        return 0;
    }
    const rocco::DeviceBuffer *all[] = {&solver->dev_tasks, &solver->dev_params, &solver->dev_results, &solver->dev_bits, &solver->dev_misc,
                                        &solver->dev_median_partials, &solver->dev_solution, &solver->dev_maps, &solver->dev_frozen,
                                        &solver->dev_lean_pool, &solver->dev_lean_round, &solver->dev_lean_look, &solver->dev_lean_desc,
                                        &solver->dev_lean_wcap, &solver->dev_chain};
    long long total = 0;
    for (const rocco::DeviceBuffer *b : all) {
        total += (long long)b->bytes;
    }
    return total;
}

int rocco_hip_count_path_reserve(rocco_hip_solver *solver, size_t count, const size_t *rows, const size_t *cols, double penalty_lambda,
                                 void *stream)
{
    return rocco_hip_count_path_reserve_ex(solver, count, rows, cols, penalty_lambda, 0, stream);
}

int rocco_hip_count_path_reserve_ex(rocco_hip_solver *solver, size_t count, const size_t *rows, const size_t *cols, double penalty_lambda,
                                    int sweeps_scratch_is_the_callers, void *stream)
{
    if (solver == nullptr || (count > 0 && (rows == nullptr || cols == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    size_t misc = (sweeps_scratch_is_the_callers != 0) ? 0 : whittaker_batch_scratch_bytes(rows, cols, count);
    size_t stage_single = 0, total_rows = 0, most_rows = 0, longest = 0;
    for (size_t i = 0; i < count; ++i) {
        if (rows[i] == 0 || cols[i] == 0) {
            continue;
        }
        misc = std::max(misc, wls_scratch_bytes(rows[i], cols[i], 31, true));
        misc = std::max(misc, wls_scratch_bytes(rows[i], cols[i], 31, false));
        misc = std::max(misc, log_scale_scratch_bytes(rows[i], cols[i]));
        if (sweeps_scratch_is_the_callers == 0) {
            misc = std::max(misc, whittaker_batch_scratch_bytes(&rows[i], &cols[i], 1));
        }
        stage_single = std::max(stage_single, whittaker_batch_stage_bytes(&rows[i], &cols[i], 1));
        total_rows += rows[i];
        most_rows = std::max(most_rows, rows[i]);
        longest = std::max(longest, cols[i]);
    }
    int rc;
    if ((rc = solver->dev_misc.reserve(misc)) != ROCCO_HIP_OK) return rc;
    if ((rc = solver->dev_tasks.reserve(total_rows * sizeof(WlsRollingTask) + 256)) != ROCCO_HIP_OK) return rc;
    if ((rc = solver->host_stage.reserve(std::max(std::max(whittaker_batch_stage_bytes(rows, cols, count), stage_single), total_rows * sizeof(WlsRollingTask) + 256))) != ROCCO_HIP_OK) return rc;
    if ((rc = solver->host_back.reserve(256 + most_rows * sizeof(int))) != ROCCO_HIP_OK) return rc;
    if ((rc = solver->dev_results.reserve(256)) != ROCCO_HIP_OK) return rc;
    if (penalty_lambda > 0.0 && (rc = ensure_whittaker_factor(solver, longest, penalty_lambda, (hipStream_t)stream)) != ROCCO_HIP_OK) return rc;
    return ROCCO_HIP_OK;
}

int rocco_hip_score_centered_wls_f64(rocco_hip_solver *solver, const double *centered_dev, size_t K, size_t n,
                                     double lower_bound_z, double prior_df, double min_effect, int use_min_effect,
                                     int spatial_window, double precision_floor_ratio, double *mean_dev,
                                     double *raw_var_dev, double *prior_var_dev, double *mod_var_dev, double *se_dev,
                                     double *scores_dev, double *df_out, int *window_out, void *stream)
{
    return rocco_hip_score_centered_wls_given_variances_f64(solver, centered_dev, K, n, lower_bound_z, prior_df, min_effect,
                                                            use_min_effect, spatial_window, precision_floor_ratio, nullptr, mean_dev,
                                                            raw_var_dev, prior_var_dev, mod_var_dev, se_dev, scores_dev, df_out,
                                                            window_out, stream);
}

int rocco_hip_score_centered_wls_given_variances_f64(rocco_hip_solver *solver, const double *centered_dev, size_t K, size_t n,
                                                     double lower_bound_z, double prior_df, double min_effect, int use_min_effect,
                                                     int spatial_window, double precision_floor_ratio, const double *variances_dev,
                                                     double *mean_dev, double *raw_var_dev, double *prior_var_dev, double *mod_var_dev,
                                                     double *se_dev, double *scores_dev, double *df_out, int *window_out, void *stream)
{
    // argument checks of rocco_score_centered_wls_f64 (wls_backend.c:770-776)
    if (solver == nullptr || centered_dev == nullptr || mean_dev == nullptr || raw_var_dev == nullptr ||
        prior_var_dev == nullptr || mod_var_dev == nullptr || se_dev == nullptr || scores_dev == nullptr || K == 0 ||
        n == 0 || n > (size_t)0x7fffffff) {
        set_last_error("rocco_hip_score_centered_wls_f64: null buffer, empty matrix or more than 2^31-1 loci");
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    int rc;
    if ((rc = solver->dev_misc.reserve(wls_scratch_bytes(K, n, spatial_window, variances_dev == nullptr))) != ROCCO_HIP_OK) {
        return rc;
    }
    if ((rc = solver->host_back.reserve(256 + K * sizeof(int))) != ROCCO_HIP_OK) {  // the non-finite flag + one flag per row
        return rc;
    }
    if (variances_dev != nullptr && wls_spatial_window(n, spatial_window) > wls_max_window()) {
        set_last_error("rocco_hip_score_centered_wls_given_variances_f64: windows above 63 loci compute their own variances");
        return ROCCO_HIP_EINVAL;
    }
    wls_set_rolling_group_min(solver->rolling_group_min);
    return launch_score_centered_wls(centered_dev, K, n, lower_bound_z, prior_df, min_effect, use_min_effect,
                                     spatial_window, precision_floor_ratio, mean_dev, raw_var_dev, prior_var_dev,
                                     mod_var_dev, se_dev, scores_dev, solver->dev_misc.ptr, df_out, window_out,
                                     (hipStream_t)stream, (int *)solver->host_back.ptr, variances_dev, &solver->wls_sorted_rows);
}

int rocco_hip_wls_sorted_rows(const rocco_hip_solver *solver) { return solver != nullptr ? solver->wls_sorted_rows : -1; }

int rocco_hip_log2_selfcheck(rocco_hip_solver *solver, int family, unsigned long long seed, unsigned long long first, size_t count,
                             unsigned long long *mismatches_out, void *stream)
{
    if (solver == nullptr || mismatches_out == nullptr || family < 0 || family > 4 || count > ((size_t)1 << 39)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    int rc;
    if ((rc = solver->dev_results.reserve(256)) != ROCCO_HIP_OK) return rc;
    if ((rc = solver->host_back.reserve(256)) != ROCCO_HIP_OK) return rc;
    unsigned long long *out = (unsigned long long *)solver->dev_results.ptr;
    ROCCO_HIP_TRY(hipMemsetAsync(out, 0, sizeof(unsigned long long), (hipStream_t)stream));
    if ((rc = launch_log2_selfcheck(family, seed, first, count, out, (hipStream_t)stream)) != ROCCO_HIP_OK) return rc;
    ROCCO_HIP_TRY(hipMemcpyAsync(solver->host_back.ptr, out, sizeof(unsigned long long), hipMemcpyDeviceToHost, (hipStream_t)stream));
    ROCCO_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    *mismatches_out = *(unsigned long long *)solver->host_back.ptr;
    return ROCCO_HIP_OK;
}

int rocco_hip_log_scale_f64(rocco_hip_solver *solver, const double *values_dev, size_t count, double pseudocount, double *out_dev,
                            void *stream)
{
    if (solver == nullptr || (count > 0 && (values_dev == nullptr || out_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    int rc = solver->dev_results.reserve(256);
    if (rc != ROCCO_HIP_OK) return rc;
    int *bad = (int *)solver->dev_results.ptr;
    ROCCO_HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), (hipStream_t)stream));
    if ((rc = launch_log_scale(values_dev, out_dev, count, pseudocount, bad, (hipStream_t)stream)) != ROCCO_HIP_OK) return rc;
    if ((rc = solver->host_back.reserve(256)) != ROCCO_HIP_OK) return rc;
    int &bad_host = *(int *)solver->host_back.ptr;  // (pinned: see launch_score_centered_wls)
    bad_host = 0;
    ROCCO_HIP_TRY(hipMemcpyAsync(&bad_host, bad, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    ROCCO_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (bad_host != 0) {
        set_last_error("`chrom_matrix` contains non-finite values");
        return ROCCO_HIP_EINVAL;
    }
    return ROCCO_HIP_OK;
}

int rocco_hip_log_scale_center_rows_f64(rocco_hip_solver *solver, const double *counts_dev, size_t K, size_t n,
                                        double pseudocount, int apply_log2, double *centered_out_dev,
                                        double *row_offsets_out_dev, void *stream)
{
    if (solver == nullptr || counts_dev == nullptr || centered_out_dev == nullptr || K == 0 || n == 0 ||
        n > (size_t)0x7fffffff) {
        set_last_error("rocco_hip_log_scale_center_rows_f64: null buffer, empty matrix or more than 2^31-1 loci");
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    int rc;
    if ((rc = solver->dev_misc.reserve(log_scale_scratch_bytes(K, n))) != ROCCO_HIP_OK) {
        return rc;
    }
    if ((rc = solver->host_back.reserve(256)) != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_log_scale_center_rows(counts_dev, K, n, pseudocount, apply_log2, centered_out_dev, row_offsets_out_dev,
                                        solver->dev_misc.ptr, (hipStream_t)stream, (int *)solver->host_back.ptr);
}

int rocco_hip_log_scale_row_offsets_f64(rocco_hip_solver *solver, const double *counts_dev, size_t K, size_t n,
                                        double pseudocount, int apply_log2, double *log_out_dev, double *row_offsets_out_dev,
                                        void *stream)
{
    if (solver == nullptr || counts_dev == nullptr || log_out_dev == nullptr || row_offsets_out_dev == nullptr || K == 0 || n == 0 ||
        n > (size_t)0x7fffffff) {
        set_last_error("rocco_hip_log_scale_row_offsets_f64: null buffer, empty matrix or more than 2^31-1 loci");
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    int rc;
    if ((rc = solver->dev_misc.reserve(log_scale_scratch_bytes(K, n))) != ROCCO_HIP_OK) {
        return rc;
    }
    if ((rc = solver->host_back.reserve(256)) != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_log_scale_center_rows(counts_dev, K, n, pseudocount, apply_log2, log_out_dev, row_offsets_out_dev,
                                        solver->dev_misc.ptr, (hipStream_t)stream, (int *)solver->host_back.ptr, 0);
}

int rocco_hip_subtract_finite_f64(rocco_hip_solver *solver, const double *a_dev, const double *b_dev, double *out_dev,
                                  size_t count, void *stream)
{
    if (solver == nullptr || ((a_dev == nullptr || b_dev == nullptr || out_dev == nullptr) && count > 0)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    int rc = solver->dev_results.reserve(256);
    if (rc != ROCCO_HIP_OK) return rc;
    if ((rc = solver->host_back.reserve(256)) != ROCCO_HIP_OK) return rc;
    int *bad = (int *)solver->dev_results.ptr;
    ROCCO_HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), (hipStream_t)stream));
    if ((rc = launch_subtract(a_dev, b_dev, out_dev, count, (hipStream_t)stream, bad)) != ROCCO_HIP_OK) return rc;
    int &bad_host = *(int *)solver->host_back.ptr;
    bad_host = 0;
    ROCCO_HIP_TRY(hipMemcpyAsync(&bad_host, bad, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    ROCCO_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (bad_host != 0) {
        set_last_error("Local baseline fit produced non-finite values");
        return ROCCO_HIP_EINVAL;
    }
    return ROCCO_HIP_OK;
}

int rocco_hip_subtract_f64(rocco_hip_solver *solver, const double *a_dev, const double *b_dev, double *out_dev,
                           size_t count, void *stream)
{
    if (solver == nullptr || ((a_dev == nullptr || b_dev == nullptr || out_dev == nullptr) && count > 0)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_subtract(a_dev, b_dev, out_dev, count, (hipStream_t)stream);
}

int rocco_hip_narrowpeak_summit_offsets(rocco_hip_solver *solver, const int64_t *intervals_dev, size_t n_intervals,
                                        const int64_t *centers_dev, const double *effect_mean_dev, size_t n_mean, const int64_t *peak_start_dev,
                                        const int64_t *peak_end_dev, size_t n_peaks, int64_t *offsets_out_dev,
                                        void *stream)
{
    if (solver == nullptr ||
        (n_peaks > 0 && (peak_start_dev == nullptr || peak_end_dev == nullptr || offsets_out_dev == nullptr)) ||
        (n_intervals > 0 && intervals_dev == nullptr) || (n_mean > 0 && effect_mean_dev == nullptr)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_summit_offsets(intervals_dev, n_intervals, centers_dev, effect_mean_dev, n_mean, peak_start_dev, peak_end_dev,
                                 n_peaks, offsets_out_dev, (hipStream_t)stream);
}

int rocco_hip_union_intervals(rocco_hip_solver *solver, const int64_t *values_dev, size_t count,
                              int64_t *unique_out_dev, size_t *n_unique_out, int *fixed_step_out, void *stream)
{
    if (solver == nullptr || n_unique_out == nullptr || count > (size_t)0x7fffffff ||
        (count > 0 && (values_dev == nullptr || unique_out_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    *n_unique_out = 0;
    if (fixed_step_out != nullptr) {
        *fixed_step_out = 1;
    }
    if (count == 0) {
        return ROCCO_HIP_OK;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    int rc;
    if ((rc = solver->dev_misc.reserve(union_scratch_bytes(count))) != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_union_intervals(values_dev, count, unique_out_dev, n_unique_out, fixed_step_out, solver->dev_misc.ptr,
                                  (hipStream_t)stream);
}

int rocco_hip_scatter_tracks(rocco_hip_solver *solver, const int64_t *common_dev, size_t m,
                             const int64_t *intervals_concat_dev, const double *vals_concat_dev,
                             const size_t *offsets_host, size_t K, int out_dtype, void *matrix_out_dev, void *stream)
{
    if (solver == nullptr || offsets_host == nullptr || (out_dtype != 0 && out_dtype != 1) ||
        (K * m > 0 && (common_dev == nullptr || matrix_out_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    for (size_t k = 0; k < K; ++k) {
        if (offsets_host[k + 1] < offsets_host[k] || offsets_host[k + 1] - offsets_host[k] >= (size_t)0xffffffff) {
            return ROCCO_HIP_EINVAL;
        }
    }
    if (K > 0 && offsets_host[K] > 0 && (intervals_concat_dev == nullptr || vals_concat_dev == nullptr)) {
        return ROCCO_HIP_EINVAL;
    }
    if (K * m == 0) {
        return ROCCO_HIP_OK;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    int rc;
    if ((rc = solver->dev_misc.reserve(scatter_scratch_bytes(K, m))) != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_scatter_tracks(common_dev, m, intervals_concat_dev, vals_concat_dev, offsets_host, K, out_dtype,
                                 matrix_out_dev, solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_numpy_sum_f64(rocco_hip_solver *solver, const double *x_dev, size_t n, double *sum_out, void *stream)
{
    if (solver == nullptr || sum_out == nullptr || (n > 0 && x_dev == nullptr)) {
        return ROCCO_HIP_EINVAL;
    }
    *sum_out = 0.0;
    if (n == 0) {
        return ROCCO_HIP_OK;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    int rc;
    if ((rc = solver->dev_misc.reserve(npsum_scratch_bytes(n))) != ROCCO_HIP_OK) {
        return rc;
    }
    const int mode = 0;
    return launch_numpy_sums(x_dev, n, &mode, 1, 0.0, 1.0, 0.0, solver->dev_misc.ptr, sum_out, (hipStream_t)stream);
}

int rocco_hip_budget_null_draw_stats_f64(rocco_hip_solver *solver, const double *scores_dev, size_t n,
                                         double null_center, double null_soft_scale, double null_threshold,
                                         double *stats_out, void *stream)
{
    if (solver == nullptr || stats_out == nullptr || scores_dev == nullptr || n == 0) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    int rc;
    if ((rc = solver->dev_misc.reserve(npsum_scratch_bytes(n))) != ROCCO_HIP_OK) {
        return rc;
    }
    const int modes[4] = {1, 2, 3, 4};
    double sums[4];
    if ((rc = launch_numpy_sums(scores_dev, n, modes, 4, null_center, null_soft_scale, null_threshold,
                                solver->dev_misc.ptr, sums, (hipStream_t)stream)) != ROCCO_HIP_OK) {
        return rc;
    }
    for (int i = 0; i < 4; ++i) {
        stats_out[i] = sums[i] / (double)n;  // np.mean: the sum divided by the count
    }
    return ROCCO_HIP_OK;
}

int rocco_hip_multiply_f64(rocco_hip_solver *solver, const double *a_dev, const double *b_dev, double *out_dev,
                           size_t count, void *stream)
{
    if (solver == nullptr || ((a_dev == nullptr || b_dev == nullptr || out_dev == nullptr) && count > 0)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_multiply(a_dev, b_dev, out_dev, count, (hipStream_t)stream);
}

int rocco_hip_subtract_positive_row_f64(rocco_hip_solver *solver, const double *matrix_dev, const double *row_dev,
                                        size_t K, size_t n, double *out_dev, void *stream)
{
    if (solver == nullptr || ((matrix_dev == nullptr || row_dev == nullptr || out_dev == nullptr) && K * n > 0)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_subtract_positive_row(matrix_dev, row_dev, K, n, out_dev, (hipStream_t)stream);
}

int rocco_hip_bigwig_dense_fill_f64(rocco_hip_solver *solver, const int64_t *starts_dev, const int64_t *ends_dev,
                                    const double *vals_dev, size_t count, double const_scale, int round_digits,
                                    double *full_out_dev, size_t capacity, int64_t *first_start_out, int64_t *step_out,
                                    size_t *n_full_out, int *flags_out, void *stream)
{
    if (solver == nullptr || starts_dev == nullptr || ends_dev == nullptr || vals_dev == nullptr || count == 0 ||
        first_start_out == nullptr || step_out == nullptr || n_full_out == nullptr || flags_out == nullptr ||
        round_digits > 22 || round_digits < -22) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    int rc;
    if ((rc = solver->dev_misc.reserve(256)) != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_bigwig_dense_fill(starts_dev, ends_dev, vals_dev, count, const_scale, round_digits, full_out_dev,
                                    capacity, first_start_out, step_out, n_full_out, flags_out, solver->dev_misc.ptr,
                                    (hipStream_t)stream);
}

int rocco_hip_count_alignment_records_batch(rocco_hip_solver *solver, const int32_t *pos_dev, const int32_t *end_dev,
                                            const int32_t *isize_dev, const uint16_t *flag_dev, const uint8_t *mapq_dev,
                                            const uint8_t *mate_same_dev, const int64_t *rec_offsets_host, size_t K,
                                            const rocco_hip_count_options *options_host,
                                            const rocco_hip_count_region *regions_host, const int64_t *out_offsets_host,
                                            int accumulate, float *out_dev, int64_t *max_magnitude_out_host, void *stream)
{
    if (solver == nullptr || K == 0 || K >= (size_t)0x7fffffff || rec_offsets_host == nullptr || options_host == nullptr ||
        regions_host == nullptr || out_offsets_host == nullptr || out_dev == nullptr || max_magnitude_out_host == nullptr) {
        return ROCCO_HIP_EINVAL;
    }
    if (rec_offsets_host[K] > rec_offsets_host[0] &&
        (pos_dev == nullptr || end_dev == nullptr || isize_dev == nullptr || flag_dev == nullptr || mapq_dev == nullptr ||
         mate_same_dev == nullptr)) {
        return ROCCO_HIP_EINVAL;
    }
    const size_t bytes = count_alignment_scratch_bytes(rec_offsets_host, K, options_host, regions_host, out_offsets_host);
    if (const int rc = enter_record_call(solver, bytes); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_count_alignment_records(pos_dev, end_dev, isize_dev, flag_dev, mapq_dev, mate_same_dev, rec_offsets_host, K,
                                          options_host, regions_host, out_offsets_host, accumulate, out_dev,
                                          max_magnitude_out_host, solver->dev_misc.ptr, (hipStream_t)stream);
}

void rocco_hip_count_alignment_shape(int *shape_out)
{
    shape_out[0] = ROCCO_COUNT_CHUNK_RECORDS;
    shape_out[1] = ROCCO_COUNT_MAX_GRID;
    shape_out[2] = ROCCO_COUNT_SCAN_TILE;
    shape_out[3] = ROCCO_COUNT_WINDOW_BINS;
}

int rocco_hip_alignment_chrom_range(rocco_hip_solver *solver, const int32_t *pos_dev, const int32_t *end_dev,
                                    const uint16_t *flag_dev, size_t n, int64_t chrom_len, int flag_exclude,
                                    int64_t *start_out, int64_t *end_out, void *stream)
{
    if (solver == nullptr || start_out == nullptr || end_out == nullptr || chrom_len < 0 ||
        (n > 0 && (pos_dev == nullptr || end_dev == nullptr || flag_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, 256); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_alignment_chrom_range(pos_dev, end_dev, flag_dev, n, chrom_len, flag_exclude, start_out, end_out,
                                        solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_alignment_count_tail_f64(rocco_hip_solver *solver, const float *counts_dev, size_t n, double norm_scale,
                                       int scale_by_step, double step, double const_scale, int round_digits,
                                       double *vals_out_dev, int64_t *first_out, int64_t *last_out, void *stream)
{
    if (solver == nullptr || first_out == nullptr || last_out == nullptr || round_digits > 22 || round_digits < -22 ||
        (n > 0 && (counts_dev == nullptr || vals_out_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, 256); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_alignment_count_tail(counts_dev, n, norm_scale, scale_by_step, step, const_scale, round_digits, vals_out_dev,
                                       first_out, last_out, solver->dev_misc.ptr, (hipStream_t)stream);
}

// ccounts_getChromRange per file (rocco/readtracks.py:439-446), K files in one launch
int rocco_hip_alignment_chrom_range_batch(rocco_hip_solver *solver, const int32_t *pos_dev, const int32_t *end_dev,
                                          const uint16_t *flag_dev, const int64_t *rec_offsets_host, size_t K, int64_t chrom_len,
                                          int flag_exclude, int64_t *range_out_host, void *stream)
{
    if (solver == nullptr || K == 0 || K >= (size_t)0x7fffffff || rec_offsets_host == nullptr || range_out_host == nullptr ||
        chrom_len < 0) {
        return ROCCO_HIP_EINVAL;
    }
    if (rec_offsets_host[K] > rec_offsets_host[0] && (pos_dev == nullptr || end_dev == nullptr || flag_dev == nullptr)) {
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, chrom_range_batch_scratch_bytes(K)); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_alignment_chrom_range_batch(pos_dev, end_dev, flag_dev, rec_offsets_host, K, chrom_len, flag_exclude,
                                              range_out_host, solver->dev_misc.ptr, (hipStream_t)stream);
}

// the counting and the positive support of every file (rocco/readtracks.py:475-512), one wait
int rocco_hip_track_supports(rocco_hip_solver *solver, const int32_t *pos_dev, const int32_t *end_dev, const int32_t *isize_dev,
                             const uint16_t *flag_dev, const uint8_t *mapq_dev, const uint8_t *mate_same_dev,
                             const int64_t *rec_offsets_host, size_t K, const rocco_hip_count_options *options_host,
                             const rocco_hip_count_region *regions_host, const int64_t *out_offsets_host,
                             const double *norm_scale_host, int scale_by_step, double step, double const_scale, float *out_dev,
                             int64_t *max_magnitude_out_host, int64_t *support_out_host, void *stream)
{
    if (solver == nullptr || K == 0 || K >= (size_t)0x7fffffff || rec_offsets_host == nullptr || options_host == nullptr ||
        regions_host == nullptr || out_offsets_host == nullptr || norm_scale_host == nullptr || out_dev == nullptr ||
        max_magnitude_out_host == nullptr || support_out_host == nullptr) {
        return ROCCO_HIP_EINVAL;
    }
    if (rec_offsets_host[K] > rec_offsets_host[0] &&
        (pos_dev == nullptr || end_dev == nullptr || isize_dev == nullptr || flag_dev == nullptr || mapq_dev == nullptr ||
         mate_same_dev == nullptr)) {
        return ROCCO_HIP_EINVAL;
    }
    const size_t bytes = track_supports_scratch_bytes(rec_offsets_host, K, options_host, regions_host, out_offsets_host);
    if (const int rc = enter_record_call(solver, bytes); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_track_supports(pos_dev, end_dev, isize_dev, flag_dev, mapq_dev, mate_same_dev, rec_offsets_host, K, options_host,
                                 regions_host, out_offsets_host, norm_scale_host, scale_by_step, step, const_scale, out_dev,
                                 max_magnitude_out_host, support_out_host, solver->dev_misc.ptr, (hipStream_t)stream);
}

// the trim and np.round per file (rocco/readtracks.py:505-518) and the union, zeros and scatter over the files (601-633)
int rocco_hip_track_matrix_fill(rocco_hip_solver *solver, const float *counts_dev, size_t counts_len, const int64_t *rows_dev,
                                size_t n_rows, const int64_t *segs_dev, size_t n_segs, size_t m, int scale_by_step, double step,
                                double const_scale, int round_digits, int out_dtype, void *matrix_out_dev, void *stream)
{
    if (solver == nullptr || counts_dev == nullptr || rows_dev == nullptr || segs_dev == nullptr || matrix_out_dev == nullptr ||
        n_rows == 0 || n_segs == 0 || m == 0 || n_rows >= (size_t)0x7fffffff || n_segs >= (size_t)0x7fffffff ||
        m >= ((size_t)1 << 40) || round_digits > 22 || round_digits < -22 || (out_dtype != 0 && out_dtype != 1)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device));
    (void)hipGetLastError();
    return launch_track_matrix_fill(counts_dev, counts_len, rows_dev, n_rows, segs_dev, n_segs, m, scale_by_step, step, const_scale,
                                    round_digits, out_dtype, matrix_out_dev, (hipStream_t)stream);
}

// (no reference line: the sizes at which track_matrix.hip's kernel changes path, for the tests)
void rocco_hip_track_matrix_shape(int *out)
{
    out[0] = ROCCO_TRACK_MATRIX_THREADS;
    out[1] = ROCCO_TRACK_MATRIX_UNIT;
    out[2] = ROCCO_TRACK_MATRIX_MAX_GRID;
    out[3] = ROCCO_TRACK_MATRIX_ROW_WORDS;
}

int rocco_hip_count_alignment_intervals_batch(rocco_hip_solver *solver, const int32_t *pos_dev, const int32_t *end_dev,
                                              const int32_t *isize_dev, const uint16_t *flag_dev, const uint8_t *mapq_dev,
                                              const uint8_t *mate_same_dev, const int64_t *rec_offsets_host, size_t F, size_t C,
                                              const rocco_hip_count_options *options_host, const int32_t *contig_id_dev,
                                              const int32_t *start_dev, const int32_t *end_region_dev, size_t P, int32_t *out_dev,
                                              int32_t *track_facts_out_host, void *stream)
{
    if (solver == nullptr || F == 0 || C == 0 || P == 0 || rec_offsets_host == nullptr || options_host == nullptr ||
        contig_id_dev == nullptr || start_dev == nullptr || end_region_dev == nullptr || out_dev == nullptr ||
        track_facts_out_host == nullptr) {
        return ROCCO_HIP_EINVAL;
    }
    const size_t bytes = count_intervals_scratch_bytes(rec_offsets_host, F, C, P);
    if (bytes == 0) {  // (before rec_offsets_host[F * C] is read: F * C may be what was refused)
        return ROCCO_HIP_EINVAL;
    }
    if (rec_offsets_host[F * C] > rec_offsets_host[0] &&
        (pos_dev == nullptr || end_dev == nullptr || isize_dev == nullptr || flag_dev == nullptr || mapq_dev == nullptr ||
         mate_same_dev == nullptr)) {
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, bytes); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_count_alignment_intervals(pos_dev, end_dev, isize_dev, flag_dev, mapq_dev, mate_same_dev, rec_offsets_host, F, C,
                                            options_host, contig_id_dev, start_dev, end_region_dev, P, out_dev,
                                            track_facts_out_host, solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_count_alignment_intervals_sets(rocco_hip_solver *solver, const int32_t *pos_dev, const int32_t *end_dev,
                                             const int32_t *isize_dev, const uint16_t *flag_dev, const uint8_t *mapq_dev,
                                             const uint8_t *mate_same_dev, const int64_t *rec_offsets_host, size_t F, size_t C,
                                             const rocco_hip_count_options *options_host, size_t S, const int32_t *set_id_dev,
                                             const int32_t *contig_id_dev, const int32_t *start_dev, const int32_t *end_region_dev,
                                             const int64_t *row_dev, size_t P, int32_t *out_dev, size_t out_rows,
                                             size_t out_stride, size_t col0, int32_t *track_facts_out_host, void *stream)
{
    if (solver == nullptr || F == 0 || C == 0 || P == 0 || rec_offsets_host == nullptr || options_host == nullptr ||
        set_id_dev == nullptr || contig_id_dev == nullptr || start_dev == nullptr || end_region_dev == nullptr ||
        row_dev == nullptr || out_dev == nullptr || track_facts_out_host == nullptr || S == 0 ||
        S > (size_t)ROCCO_COUNT_INTERVALS_MAX_SETS || out_rows == 0 || col0 > out_stride || F > out_stride - col0) {
        return ROCCO_HIP_EINVAL;
    }
    const size_t bytes = count_intervals_sets_scratch_bytes(rec_offsets_host, F, C, P);
    if (bytes == 0) {  // (before rec_offsets_host[F * C] is read: F * C may be what was refused)
        return ROCCO_HIP_EINVAL;
    }
    if (rec_offsets_host[F * C] > rec_offsets_host[0] &&
        (pos_dev == nullptr || end_dev == nullptr || isize_dev == nullptr || flag_dev == nullptr || mapq_dev == nullptr ||
         mate_same_dev == nullptr)) {
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, bytes); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_count_alignment_intervals_sets(pos_dev, end_dev, isize_dev, flag_dev, mapq_dev, mate_same_dev, rec_offsets_host, F,
                                                 C, options_host, S, set_id_dev, contig_id_dev, start_dev, end_region_dev, row_dev,
                                                 P, out_dev, out_rows, out_stride, col0, track_facts_out_host,
                                                 solver->dev_misc.ptr, (hipStream_t)stream);
}

void rocco_hip_count_intervals_shape(int *shape_out)
{
    shape_out[0] = ROCCO_COUNT_INTERVALS_UNIT;
    shape_out[1] = ROCCO_COUNT_INTERVALS_MAX_GRID;
    shape_out[2] = ROCCO_COUNT_INTERVALS_WAVES_PER_GROUP;
}

int rocco_hip_record_flag_facts(rocco_hip_solver *solver, const int32_t *pos_dev, const uint16_t *flag_dev,
                                const int64_t *rec_offsets_host, size_t T, int64_t *mapped_out_host, int32_t *unsorted_out_host,
                                void *stream)
{
    if (solver == nullptr || T == 0 || T >= (size_t)0x7fffffff || rec_offsets_host == nullptr || mapped_out_host == nullptr ||
        unsorted_out_host == nullptr || (rec_offsets_host[T] > rec_offsets_host[0] && (pos_dev == nullptr || flag_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, record_flag_facts_scratch_bytes(T)); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_record_flag_facts(pos_dev, flag_dev, rec_offsets_host, T, mapped_out_host, unsorted_out_host, solver->dev_misc.ptr,
                                    (hipStream_t)stream);
}

int rocco_hip_fragment_block_centers(rocco_hip_solver *solver, const int32_t *pos_dev, const uint16_t *flag_dev,
                                     const int64_t *rec_offsets_host, size_t T, const int64_t *contig_len_host, int flag_exclude,
                                     int max_iterations, int block_size, int rolling_chunk_size, int32_t *centers_out_host,
                                     int32_t *center_count_out_host, const int64_t *chunk_offsets_host, int32_t *density_out_dev,
                                     int32_t *rank_out_dev, void *stream)
{
    if (solver == nullptr || T == 0 || T >= (size_t)0x7fffffff || rec_offsets_host == nullptr || contig_len_host == nullptr ||
        centers_out_host == nullptr || center_count_out_host == nullptr ||
        (rec_offsets_host[T] > rec_offsets_host[0] && (pos_dev == nullptr || flag_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    const size_t bytes = fragment_block_centers_scratch_bytes(rec_offsets_host, T, contig_len_host, block_size, rolling_chunk_size);
    if (const int rc = enter_record_call(solver, bytes); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_fragment_block_centers(pos_dev, flag_dev, rec_offsets_host, T, contig_len_host, flag_exclude, max_iterations, block_size,
                                         rolling_chunk_size, centers_out_host, center_count_out_host, chunk_offsets_host,
                                         density_out_dev, rank_out_dev, solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_strand_xcorr_blocks(rocco_hip_solver *solver, const int32_t *pos_dev, const int32_t *end_dev, const uint16_t *flag_dev,
                                  const int64_t *rec_offsets_host, size_t T, const int32_t *block_track_host,
                                  const int64_t *block_start_host, size_t n_blocks, const int32_t *min_lag_host, int flag_exclude,
                                  int block_size, int max_insert_size, int lag_step, int32_t *best_lag_out_host,
                                  double *best_score_out_host, int32_t *fwd_sum_out_host, int32_t *rev_sum_out_host, void *stream)
{
    if (solver == nullptr || T == 0 || T >= (size_t)0x7fffffff || n_blocks == 0 || n_blocks >= (size_t)0x7fffffff ||
        rec_offsets_host == nullptr || block_track_host == nullptr || block_start_host == nullptr || min_lag_host == nullptr ||
        best_lag_out_host == nullptr || best_score_out_host == nullptr || fwd_sum_out_host == nullptr || rev_sum_out_host == nullptr ||
        (rec_offsets_host[T] > rec_offsets_host[0] && (pos_dev == nullptr || end_dev == nullptr || flag_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, strand_xcorr_scratch_bytes(T, n_blocks)); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_strand_xcorr_blocks(pos_dev, end_dev, flag_dev, rec_offsets_host, T, block_track_host, block_start_host, n_blocks,
                                      min_lag_host, flag_exclude, block_size, max_insert_size, lag_step, best_lag_out_host,
                                      best_score_out_host, fwd_sum_out_host, rev_sum_out_host, solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_template_lengths(rocco_hip_solver *solver, const int32_t *isize_dev, const uint16_t *flag_dev, const uint8_t *mate_same_dev,
                               const int64_t *rec_offsets_host, size_t T, const int32_t *min_insert_host, int flag_exclude,
                               int max_insert_size, int32_t *lengths_tmp_dev, int32_t *lengths_out_dev, int64_t *count_out_host,
                               void *stream)
{
    if (solver == nullptr || T == 0 || T >= (size_t)0x7fffffff || rec_offsets_host == nullptr || min_insert_host == nullptr ||
        count_out_host == nullptr ||
        (rec_offsets_host[T] > rec_offsets_host[0] && (isize_dev == nullptr || flag_dev == nullptr || mate_same_dev == nullptr ||
                                                       lengths_tmp_dev == nullptr || lengths_out_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    const size_t bytes = template_lengths_scratch_bytes(rec_offsets_host, T);
    if (const int rc = enter_record_call(solver, bytes); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_template_lengths(isize_dev, flag_dev, mate_same_dev, rec_offsets_host, T, min_insert_host, flag_exclude,
                                   max_insert_size, lengths_tmp_dev, lengths_out_dev, count_out_host, solver->dev_misc.ptr,
                                   (hipStream_t)stream);
}

void rocco_hip_fragment_length_shape(int *shape_out)
{
    shape_out[0] = ROCCO_FRAGMENT_THREADS;
    shape_out[1] = ROCCO_FRAGMENT_DENSITY_RECORDS;
    shape_out[2] = ROCCO_FRAGMENT_DENSITY_WINDOW;
    shape_out[3] = ROCCO_FRAGMENT_MAX_BLOCK_SIZE;
}

int rocco_hip_bam_walk_records(rocco_hip_solver *solver, const uint8_t *bytes_dev, size_t n_bytes, int64_t entry0, int n_ref,
                               size_t segment_bytes, int guess_mode, int64_t *offsets_out_dev, size_t capacity,
                               int64_t *segment_entry_out_dev, int64_t *report_out_host, void *stream)
{
    if (solver == nullptr || report_out_host == nullptr || n_ref < 0 || entry0 < 0 || (uint64_t)entry0 > (uint64_t)n_bytes ||
        (guess_mode != 0 && guess_mode != 1) || (n_bytes > 0 && bytes_dev == nullptr) || (capacity > 0 && offsets_out_dev == nullptr)) {
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, bam_walk_scratch_bytes(n_bytes, segment_bytes)); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_bam_walk_records(bytes_dev, n_bytes, entry0, n_ref, segment_bytes, guess_mode, offsets_out_dev, capacity,
                                   segment_entry_out_dev, report_out_host, solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_bam_record_fields(rocco_hip_solver *solver, const uint8_t *bytes_dev, size_t n_bytes, const int64_t *offsets_dev, size_t n,
                                int n_ref, int32_t *tid_out_dev, int32_t *pos_out_dev, int32_t *end_out_dev, int32_t *isize_out_dev,
                                uint16_t *flag_out_dev, uint8_t *mapq_out_dev, uint8_t *mate_same_out_dev, int32_t *qlen_out_dev,
                                int64_t *contig_first_out_host, int64_t *report_out_host, void *stream)
{
    if (solver == nullptr || n_ref < 0 || n >= ((size_t)1 << 55) || contig_first_out_host == nullptr || report_out_host == nullptr ||
        (n > 0 && (bytes_dev == nullptr || offsets_dev == nullptr || tid_out_dev == nullptr || pos_out_dev == nullptr ||
                   end_out_dev == nullptr || isize_out_dev == nullptr || flag_out_dev == nullptr || mapq_out_dev == nullptr ||
                   mate_same_out_dev == nullptr || qlen_out_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, bam_record_fields_scratch_bytes(n_ref)); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_bam_record_fields(bytes_dev, n_bytes, offsets_dev, n, n_ref, tid_out_dev, pos_out_dev, end_out_dev, isize_out_dev,
                                    flag_out_dev, mapq_out_dev, mate_same_out_dev, qlen_out_dev, contig_first_out_host, report_out_host,
                                    solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_bam_stream_firsts(rocco_hip_solver *solver, const int64_t *offsets_dev, const int32_t *tid_dev, size_t n,
                                const int64_t *bounds_host, const int32_t *expect_tid_host, size_t n_streams, int64_t *firsts_out_host,
                                int64_t *report_out_host, void *stream)
{
    if (solver == nullptr || bounds_host == nullptr || expect_tid_host == nullptr || firsts_out_host == nullptr || report_out_host == nullptr ||
        n_streams < 1 || n_streams >= ((size_t)1 << 24) || n >= ((size_t)1 << 55) || (n > 0 && (offsets_dev == nullptr || tid_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    for (size_t j = 0; j < n_streams; ++j) {
        if (bounds_host[j] < 0 || bounds_host[j] > bounds_host[j + 1]) {
            return ROCCO_HIP_EINVAL;
        }
    }
    if (const int rc = enter_record_call(solver, bam_stream_firsts_scratch_bytes(n_streams)); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_bam_stream_firsts(offsets_dev, tid_dev, n, bounds_host, expect_tid_host, n_streams, firsts_out_host, report_out_host,
                                    solver->dev_misc.ptr, (hipStream_t)stream);
}

void rocco_hip_bam_shape(int *shape_out)
{
    shape_out[0] = ROCCO_BAM_GUESS_DEPTH;
    shape_out[1] = ROCCO_BAM_SEGMENT_BYTES;
    shape_out[2] = ROCCO_BAM_THREADS;
}

int rocco_hip_bgzf_inflate(rocco_hip_solver *solver, const uint8_t *comp_dev, size_t n_comp, const int64_t *table_dev, size_t n_blocks,
                           uint8_t *out_dev, size_t n_out, int32_t *status_out_dev, int64_t *report_out_host, void *stream)
{
    return inflate_on_device<BgzfFraming>(solver, comp_dev, n_comp, table_dev, n_blocks, out_dev, n_out, status_out_dev, nullptr,
                                          report_out_host, stream);
}

int rocco_hip_bgzf_inflate_host(rocco_hip_solver *, const uint8_t *comp, size_t n_comp, const int64_t *table, size_t n_blocks, uint8_t *out,
                                size_t n_out, int32_t *status_out, int64_t *report_out)
{
    return inflate_on_host<BgzfFraming>(comp, n_comp, table, n_blocks, out, n_out, status_out, nullptr, report_out);
}

void rocco_hip_bgzf_shape(int *shape_out)
{
    shape_out[0] = ROCCO_BGZF_THREADS;
    shape_out[1] = ROCCO_BGZF_TABLE_COLUMNS;
    shape_out[2] = ROCCO_BGZF_MAX_ISIZE;
    shape_out[3] = ROCCO_BGZF_STREAM_REASONS;
}

int rocco_hip_zlib_inflate(rocco_hip_solver *solver, const uint8_t *comp_dev, size_t n_comp, const int64_t *table_dev, size_t n_blocks,
                           uint8_t *out_dev, size_t n_out, int32_t *status_out_dev, int64_t *produced_out_dev, int64_t *report_out_host,
                           void *stream)
{
    return inflate_on_device<ZlibFraming>(solver, comp_dev, n_comp, table_dev, n_blocks, out_dev, n_out, status_out_dev, produced_out_dev,
                                          report_out_host, stream);
}

int rocco_hip_zlib_inflate_host(rocco_hip_solver *, const uint8_t *comp, size_t n_comp, const int64_t *table, size_t n_blocks, uint8_t *out,
                                size_t n_out, int32_t *status_out, int64_t *produced_out, int64_t *report_out)
{
    return inflate_on_host<ZlibFraming>(comp, n_comp, table, n_blocks, out, n_out, status_out, produced_out, report_out);
}

void rocco_hip_zlib_shape(int *shape_out)
{
    shape_out[0] = ROCCO_BGZF_THREADS;
    shape_out[1] = ROCCO_ZLIB_TABLE_COLUMNS;
    shape_out[2] = ROCCO_BGZF_MAX_ISIZE;
    shape_out[3] = ROCCO_ZLIB_HEADER_REASONS;
    shape_out[4] = ROCCO_ZLIB_MAX_GRID;
}

// what the three section entry points ask of their inputs, device or host memory alike: every pointer with a size that is
// not 0, the files' arrays sound, the per-block outputs long enough
static bool sections_args_ok(const void *slots, size_t n_slots, const void *table, const void *produced, size_t n_blocks,
                             const int64_t *file_first, const int64_t *chrom_id, const int64_t *chrom_length, size_t n_files,
                             const void *block_first, size_t n_block_first)
{
    if (n_blocks >= (size_t)0x7fffffff || n_files >= ((size_t)1 << 24) || n_slots >= ((size_t)1 << 62) || file_first == nullptr ||
        (n_files > 0 && (chrom_id == nullptr || chrom_length == nullptr)) || (n_slots > 0 && slots == nullptr) ||
        (n_blocks > 0 && (table == nullptr || produced == nullptr)) || block_first == nullptr || n_block_first < n_blocks + 1 || !section_files_ok(file_first, n_files, n_blocks)) {
        return false;
    }
    for (size_t k = 0; k < n_files; ++k) {
        if (chrom_id[k] < 0 || chrom_id[k] > 0xFFFFFFFFLL || chrom_length[k] < 0 || chrom_length[k] > 0xFFFFFFFFLL) {
            return false;
        }
    }
    return true;
}

static bool sections_status_ok(const void *status, size_t n_status, size_t n_blocks)
{
    return n_status >= n_blocks && (n_status == 0 || status != nullptr);
}

static bool sections_outputs_ok(size_t total, const void *starts, size_t n_starts, const void *ends, size_t n_ends, const void *values,
                                size_t n_values)
{
    return total < ((size_t)1 << 55) && n_starts >= total && n_ends >= total && n_values >= total && (n_starts == 0 || starts != nullptr) &&
           (n_ends == 0 || ends != nullptr) && (n_values == 0 || values != nullptr);
}

int rocco_hip_bigwig_sections_facts(rocco_hip_solver *solver, const uint8_t *slots_dev, size_t n_slots, const int64_t *table_dev,
                                    const int64_t *produced_dev, size_t n_blocks, const int64_t *file_first_host,
                                    const int64_t *chrom_id_host, const int64_t *chrom_length_host, size_t n_files, int32_t *status_out_dev,
                                    size_t n_status, int64_t *block_first_out_dev, size_t n_block_first, int64_t *file_offsets_out_host,
                                    int64_t *report_out_host, void *stream)
{
    if (solver == nullptr || file_offsets_out_host == nullptr || report_out_host == nullptr ||
        !sections_args_ok(slots_dev, n_slots, table_dev, produced_dev, n_blocks, file_first_host, chrom_id_host, chrom_length_host, n_files,
                          block_first_out_dev, n_block_first) ||
        !sections_status_ok(status_out_dev, n_status, n_blocks)) {
        set_last_error("bigwig_sections_facts: a null pointer with a size, a size too small, or file offsets that do not ascend from 0 to n_blocks");
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, bigwig_sections_scratch_bytes(n_blocks, n_files)); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_bigwig_sections_facts(slots_dev, n_slots, table_dev, produced_dev, n_blocks, file_first_host, chrom_id_host, chrom_length_host,
                                        n_files, status_out_dev, block_first_out_dev, file_offsets_out_host, report_out_host,
                                        solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_bigwig_sections_emit(rocco_hip_solver *solver, const uint8_t *slots_dev, size_t n_slots, const int64_t *table_dev,
                                   const int64_t *produced_dev, size_t n_blocks, const int64_t *file_first_host,
                                   const int64_t *chrom_id_host, const int64_t *chrom_length_host, size_t n_files,
                                   const int64_t *block_first_dev, size_t n_block_first, size_t total, int64_t *starts_out_dev, size_t n_starts,
                                   int64_t *ends_out_dev, size_t n_ends, double *values_out_dev, size_t n_values, void *stream)
{
    if (solver == nullptr ||
        !sections_args_ok(slots_dev, n_slots, table_dev, produced_dev, n_blocks, file_first_host, chrom_id_host, chrom_length_host, n_files,
                          block_first_dev, n_block_first) ||
        !sections_outputs_ok(total, starts_out_dev, n_starts, ends_out_dev, n_ends, values_out_dev, n_values)) {
        set_last_error("bigwig_sections_emit: a null pointer with a size, an output shorter than the total, or file offsets that do not ascend "
                       "from 0 to n_blocks");
        return ROCCO_HIP_EINVAL;
    }
    if (total == 0 || n_blocks == 0) {
        return ROCCO_HIP_OK;
    }
    if (const int rc = enter_record_call(solver, bigwig_sections_scratch_bytes(n_blocks, n_files)); rc != ROCCO_HIP_OK) {
        return rc;
    }
    const size_t capacity = std::min(n_starts, std::min(n_ends, n_values));
    return launch_bigwig_sections_emit(slots_dev, n_slots, table_dev, produced_dev, n_blocks, file_first_host, chrom_id_host, chrom_length_host,
                                       n_files, block_first_dev, capacity, starts_out_dev, ends_out_dev, values_out_dev, solver->dev_misc.ptr,
                                       (hipStream_t)stream);
}

int rocco_hip_bigwig_sections_host(rocco_hip_solver *, const uint8_t *slots, size_t n_slots, const int64_t *table, const int64_t *produced,
                                   size_t n_blocks, const int64_t *file_first, const int64_t *chrom_id, const int64_t *chrom_length,
                                   size_t n_files, int32_t *status_out, size_t n_status, int64_t *block_first_out, size_t n_block_first,
                                   int64_t *file_offsets_out, int64_t *starts_out, size_t n_starts, int64_t *ends_out, size_t n_ends,
                                   double *values_out, size_t n_values, int64_t *report_out)
{
    if (file_offsets_out == nullptr || report_out == nullptr ||
        !sections_args_ok(slots, n_slots, table, produced, n_blocks, file_first, chrom_id, chrom_length, n_files, block_first_out, n_block_first) ||
        !sections_status_ok(status_out, n_status, n_blocks) ||
        !sections_outputs_ok(0, starts_out, n_starts, ends_out, n_ends, values_out, n_values) ||
        ((starts_out == nullptr) != (ends_out == nullptr)) || ((starts_out == nullptr) != (values_out == nullptr))) {
        set_last_error("bigwig_sections_host: a null pointer with a size, a size too small, or file offsets that do not ascend from 0 to n_blocks");
        return ROCCO_HIP_EINVAL;
    }
    static_assert(sizeof(double) == sizeof(uint64_t), "the values are placed as bit patterns");
    if (!sections_host(slots, n_slots, table, produced, n_blocks, file_first, chrom_id, chrom_length, n_files, status_out, block_first_out,
                       file_offsets_out, starts_out, ends_out, (uint64_t *)values_out, std::min(n_starts, std::min(n_ends, n_values)),
                       report_out)) {
        set_last_error("bigwig_sections_host: the sections hold " + std::to_string(report_out[2]) + " intervals, an output has room for fewer");
        return ROCCO_HIP_EINVAL;
    }
    return ROCCO_HIP_OK;
}

void rocco_hip_bigwig_sections_shape(int *shape_out)
{
    shape_out[0] = ROCCO_BIGWIG_THREADS;
    shape_out[1] = ROCCO_BIGWIG_MAX_GRID;
    shape_out[2] = (int)kSectionHeaderBytes;
}

// ---- fragments files (row f13): the checks of every pointer and size; the launchers check what the host arrays hold ----

static bool fragfile_fields_args_ok(const void *bytes, size_t n_bytes, const void *starts, size_t n_lines, const void *expect, size_t K,
                                    const void *names, const int64_t *name_offsets, size_t n_names, const void *allow_bytes, const void *allow_offsets,
                                    size_t n_allow, const void *allow_first, const void *report)
{
    // (n_lines < 2^32: the word of the first offending line keeps the line in its upper 32 bits)
    return report != nullptr && K >= 1 && K < (size_t)0x7fffffff && n_lines < ((size_t)1 << 32) && n_bytes < ((size_t)1 << 40) && n_names < 65536 &&
           n_allow < ((size_t)1 << 40) && expect != nullptr && allow_first != nullptr && name_offsets != nullptr && starts != nullptr &&
           (n_bytes == 0 || bytes != nullptr) && (n_names == 0 || names != nullptr || name_offsets[n_names] == 0) &&
           (n_allow == 0 || (allow_bytes != nullptr && allow_offsets != nullptr));
}

int rocco_hip_fragfile_lines(rocco_hip_solver *solver, const uint8_t *bytes_dev, size_t n_bytes, size_t entry0, int64_t *starts_out_dev,
                             size_t capacity, int64_t *report_out_host, void *stream)
{
    if (solver == nullptr || report_out_host == nullptr || n_bytes >= ((size_t)1 << 40) || entry0 > n_bytes || (n_bytes > 0 && bytes_dev == nullptr)) {
        set_last_error("fragfile_lines: a null pointer with a size, entry0 beyond n_bytes, or 2^40 bytes and more");
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, fragfile_lines_scratch_bytes(n_bytes, entry0)); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_fragfile_lines(bytes_dev, n_bytes, entry0, starts_out_dev, capacity, report_out_host, solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_fragfile_fields(rocco_hip_solver *solver, const uint8_t *bytes_dev, size_t n_bytes, const int64_t *starts_dev, size_t n_lines,
                              int whole_file, const int64_t *track_first_host, const int32_t *expect_host, size_t K,
                              const uint8_t *names_host, const int64_t *name_offsets_host, size_t n_names, const uint8_t *allow_bytes_dev,
                              const int64_t *allow_offsets_dev, size_t n_allow, const int64_t *allow_first_host, int32_t *start_out_dev,
                              int32_t *end_out_dev, int32_t *weight_out_dev, int32_t *name_out_dev, uint32_t *status_out_dev,
                              int64_t *report_out_host, void *stream)
{
    if (solver == nullptr || track_first_host == nullptr ||
        !fragfile_fields_args_ok(bytes_dev, n_bytes, starts_dev, n_lines, expect_host, K, names_host, name_offsets_host, n_names, allow_bytes_dev,
                                 allow_offsets_dev, n_allow, allow_first_host, report_out_host) ||
        (n_lines > 0 && (start_out_dev == nullptr || end_out_dev == nullptr || weight_out_dev == nullptr || name_out_dev == nullptr ||
                         status_out_dev == nullptr))) {
        set_last_error("fragfile_fields: a null pointer with a size, no track, or a size beyond its limit");
        return ROCCO_HIP_EINVAL;
    }
    const size_t name_bytes = name_offsets_host[n_names] > 0 ? (size_t)name_offsets_host[n_names] : 0;
    if (const int rc = enter_record_call(solver, fragfile_fields_scratch_bytes(K, n_names, name_bytes)); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_fragfile_fields(bytes_dev, n_bytes, starts_dev, n_lines, whole_file, track_first_host, expect_host, K, names_host,
                                  name_offsets_host, n_names, allow_bytes_dev, allow_offsets_dev, n_allow, allow_first_host, start_out_dev,
                                  end_out_dev, weight_out_dev, name_out_dev, status_out_dev, report_out_host, solver->dev_misc.ptr,
                                  (hipStream_t)stream);
}

int rocco_hip_fragfile_count_batch(rocco_hip_solver *solver, const int32_t *start_dev, const int32_t *end_dev, const int32_t *weight_dev,
                                   const uint32_t *status_dev, const int64_t *line_offsets_host, size_t K,
                                   const rocco_hip_fragfile_options *options_host, const rocco_hip_count_region *regions_host,
                                   const int64_t *out_offsets_host, float *out_dev, int64_t *max_magnitude_out_host, void *stream)
{
    if (solver == nullptr || K == 0 || K >= (size_t)0x7fffffff || line_offsets_host == nullptr || options_host == nullptr ||
        regions_host == nullptr || out_offsets_host == nullptr || out_dev == nullptr || max_magnitude_out_host == nullptr) {
        return ROCCO_HIP_EINVAL;
    }
    if (line_offsets_host[K] > line_offsets_host[0] &&
        (start_dev == nullptr || end_dev == nullptr || weight_dev == nullptr || status_dev == nullptr)) {
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, fragfile_count_scratch_bytes(K, regions_host)); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_fragfile_count_batch(start_dev, end_dev, weight_dev, status_dev, line_offsets_host, K, options_host, regions_host,
                                       out_offsets_host, out_dev, max_magnitude_out_host, solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_fragfile_chrom_range_batch(rocco_hip_solver *solver, const int32_t *start_dev, const int32_t *end_dev,
                                         const uint32_t *status_dev, const int64_t *line_offsets_host, const int64_t *chrom_len_host,
                                         size_t K, int64_t *range_out_host, void *stream)
{
    if (solver == nullptr || K == 0 || K >= (size_t)0x7fffffff || line_offsets_host == nullptr || chrom_len_host == nullptr ||
        range_out_host == nullptr) {
        return ROCCO_HIP_EINVAL;
    }
    if (line_offsets_host[K] > line_offsets_host[0] && (start_dev == nullptr || end_dev == nullptr || status_dev == nullptr)) {
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, fragfile_range_scratch_bytes(K)); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_fragfile_chrom_range_batch(start_dev, end_dev, status_dev, line_offsets_host, chrom_len_host, K, range_out_host,
                                             solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_fragfile_mapped_count(rocco_hip_solver *solver, const int32_t *weight_dev, const int32_t *name_dev, const uint32_t *status_dev,
                                    size_t n_lines, int count_mode, int one_read_per_bin, uint64_t *sum_out_host, void *stream)
{
    if (solver == nullptr || sum_out_host == nullptr || n_lines >= ((size_t)1 << 40) || count_mode < 0 || count_mode > ROCCO_FRAGFILE_MODE_CENTER ||
        (n_lines > 0 && (weight_dev == nullptr || name_dev == nullptr || status_dev == nullptr))) {
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, 256); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_fragfile_mapped_count(weight_dev, name_dev, status_dev, n_lines, count_mode, one_read_per_bin, sum_out_host,
                                        solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_fragfile_host(rocco_hip_solver *, const uint8_t *bytes, size_t n_bytes, size_t entry0, int64_t *starts_out, size_t capacity,
                            int64_t *lines_report_out, int whole_file, const int64_t *track_first, const int32_t *expect, size_t K,
                            const uint8_t *names, const int64_t *name_offsets, size_t n_names, const uint8_t *allow_bytes,
                            const int64_t *allow_offsets, size_t n_allow, const int64_t *allow_first, int32_t *start_out, int32_t *end_out,
                            int32_t *weight_out, int32_t *name_out, uint32_t *status_out, int64_t *fields_report_out)
{
    if (lines_report_out == nullptr || n_bytes >= ((size_t)1 << 40) || entry0 > n_bytes || (n_bytes > 0 && bytes == nullptr)) {
        set_last_error("fragfile_host: a null pointer with a size, entry0 beyond n_bytes, or 2^40 bytes and more");
        return ROCCO_HIP_EINVAL;
    }
    if (!fragfile_lines_host(bytes, n_bytes, entry0, starts_out, capacity, lines_report_out)) {
        set_last_error("fragfile_host: the bytes hold " + std::to_string(lines_report_out[0]) + " lines, starts_out has room for " +
                       std::to_string(capacity) + " entries where one more than the lines belong");
        return ROCCO_HIP_EINVAL;
    }
    const bool fields = start_out != nullptr || end_out != nullptr || weight_out != nullptr || name_out != nullptr || status_out != nullptr;
    if (!fields) {
        return ROCCO_HIP_OK;
    }
    const size_t n_lines = (size_t)lines_report_out[0];
    const int64_t whole[2] = {0, (int64_t)n_lines};
    const size_t tracks = track_first == nullptr ? 1 : K;
    const int64_t *first = track_first == nullptr ? whole : track_first;
    if (start_out == nullptr || end_out == nullptr || weight_out == nullptr || name_out == nullptr || status_out == nullptr ||
        !fragfile_fields_args_ok(bytes, n_bytes, starts_out, n_lines, expect, tracks, names, name_offsets, n_names, allow_bytes, allow_offsets,
                                 n_allow, allow_first, fields_report_out)) {
        set_last_error("fragfile_host: the field pass needs the starts, all five outputs and its report; a null pointer with a size, or no track");
        return ROCCO_HIP_EINVAL;
    }
    for (size_t k = 0; k < tracks; ++k) {
        if (first[k] > first[k + 1] || first[0] != 0 || first[tracks] != (int64_t)n_lines || allow_first[k] > allow_first[k + 1] || allow_first[0] < 0 ||
            allow_first[tracks] > (int64_t)n_allow || expect[k] >= (int32_t)n_names) {
            set_last_error("fragfile_host: track_first must ascend from 0 to the number of lines, allow_first within the n_allow entries, expect "
                           "within the names");
            return ROCCO_HIP_EINVAL;
        }
    }
    const FragNames table = {names, name_offsets, 0, (long long)n_names};
    fragfile_fields_host(bytes, starts_out, n_lines, whole_file, first, expect, tracks, table, allow_bytes, allow_offsets, allow_first, start_out,
                         end_out, weight_out, name_out, status_out, fields_report_out);
    return ROCCO_HIP_OK;
}

void rocco_hip_fragfile_shape(int *shape_out)
{
    shape_out[0] = ROCCO_FRAGFILE_THREADS;
    shape_out[1] = ROCCO_FRAGFILE_TILE_BYTES;
    shape_out[2] = ROCCO_FRAGFILE_THREADS;
    shape_out[3] = ROCCO_FRAGFILE_LINES_MAX_GRID;
    shape_out[4] = ROCCO_FRAGFILE_FIELDS_MAX_GRID;
    shape_out[5] = ROCCO_FRAGFILE_COUNT_MAX_GRID;
}

// ---- the barcode census (row f14): the checks of every pointer, size and bound the kernels rely on --------------------------

static bool census_table_ok(const void *slots, const void *counts, size_t capacity)
{
    return slots != nullptr && counts != nullptr && capacity >= ROCCO_BARCODE_CENSUS_MIN_CAPACITY && capacity <= ((size_t)1 << 40) &&
           (capacity & (capacity - 1)) == 0;
}

int rocco_hip_barcode_census_insert(rocco_hip_solver *solver, const uint8_t *bytes_dev, size_t n_bytes, const int64_t *starts_dev, size_t n_lines,
                                    const uint8_t *allow_bytes_dev, const int64_t *allow_offsets_dev, size_t n_allow, uint64_t *slots_dev,
                                    int64_t *counts_dev, size_t capacity, uint8_t *arena_bytes_dev, size_t arena_bytes_capacity,
                                    int64_t *arena_offsets_dev, uint64_t *arena_hashes_dev, size_t arena_entries_capacity, size_t entries,
                                    size_t arena_used, uint64_t hash_mask, int64_t *report_out_host, void *stream)
{
    if (solver == nullptr || report_out_host == nullptr || !census_table_ok(slots_dev, counts_dev, capacity) || starts_dev == nullptr ||
        (n_bytes > 0 && bytes_dev == nullptr) || n_lines >= ((size_t)1 << 26) || n_bytes >= ((size_t)1 << 38) || n_allow >= ((size_t)1 << 40) ||
        (n_allow > 0 && (allow_bytes_dev == nullptr || allow_offsets_dev == nullptr)) || arena_offsets_dev == nullptr ||
        arena_hashes_dev == nullptr || (arena_bytes_capacity > 0 && arena_bytes_dev == nullptr) || entries >= ((size_t)1 << 37) ||
        arena_used >= ((size_t)1 << 40)) {
        set_last_error("barcode_census_insert: a null pointer with a size, a capacity that is no power of two from the minimum on, or a size "
                       "beyond its limit");
        return ROCCO_HIP_EINVAL;
    }
    if (capacity < 2 * (entries + n_lines) || arena_entries_capacity < entries + n_lines || arena_bytes_capacity < arena_used + n_bytes) {
        set_last_error("barcode_census_insert: the table needs 2 * (entries + n_lines) slots, the arena entries + n_lines entries and "
                       "arena_used + n_bytes bytes (" + std::to_string(capacity) + " slots, " + std::to_string(arena_entries_capacity) + " entries, " +
                       std::to_string(arena_bytes_capacity) + " bytes for " + std::to_string(entries) + " entries and " + std::to_string(n_lines) +
                       " lines)");
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, barcode_census_insert_scratch_bytes(n_lines)); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_barcode_census_insert(bytes_dev, n_bytes, starts_dev, n_lines, allow_bytes_dev, allow_offsets_dev, n_allow, slots_dev, counts_dev,
                                        capacity, arena_bytes_dev, arena_bytes_capacity, arena_offsets_dev, arena_hashes_dev, arena_entries_capacity,
                                        entries, arena_used, hash_mask, report_out_host, solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_barcode_census_rehash(rocco_hip_solver *solver, const uint64_t *slots_dev, const int64_t *counts_dev, size_t capacity,
                                    uint64_t *new_slots_dev, int64_t *new_counts_dev, size_t new_capacity, const uint64_t *arena_hashes_dev,
                                    size_t entries, uint64_t hash_mask, void *stream)
{
    if (solver == nullptr || !census_table_ok(slots_dev, counts_dev, capacity) || !census_table_ok(new_slots_dev, new_counts_dev, new_capacity) ||
        new_capacity < 2 * entries || (entries > 0 && arena_hashes_dev == nullptr) || slots_dev == new_slots_dev || counts_dev == new_counts_dev) {
        set_last_error("barcode_census_rehash: two distinct tables of a power of two of slots are required, the new one of at least 2 * entries");
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, 256); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_barcode_census_rehash(slots_dev, counts_dev, capacity, new_slots_dev, new_counts_dev, new_capacity, arena_hashes_dev, entries,
                                        hash_mask, solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_barcode_census_records(rocco_hip_solver *solver, const uint64_t *slots_dev, const int64_t *counts_dev, size_t capacity,
                                     size_t entries, int64_t *records_out_dev, void *stream)
{
    if (solver == nullptr || !census_table_ok(slots_dev, counts_dev, capacity) || (entries > 0 && records_out_dev == nullptr)) {
        set_last_error("barcode_census_records: a table of a power of two of slots and room for the entries' records are required");
        return ROCCO_HIP_EINVAL;
    }
    if (const int rc = enter_record_call(solver, 256); rc != ROCCO_HIP_OK) {
        return rc;
    }
    return launch_barcode_census_records(slots_dev, counts_dev, capacity, entries, records_out_dev, solver->dev_misc.ptr, (hipStream_t)stream);
}

int rocco_hip_barcode_census_host(rocco_hip_solver *, const uint8_t *bytes, size_t n_bytes, const uint8_t *allow_bytes, const int64_t *allow_offsets,
                                  size_t n_allow, uint64_t hash_mask, size_t initial_capacity, uint8_t *bytes_out, size_t bytes_capacity,
                                  int64_t *offsets_out, int64_t *records_out, size_t entries_capacity, int64_t *report_out)
{
    if (report_out == nullptr || n_bytes >= ((size_t)1 << 40) || (n_bytes > 0 && bytes == nullptr) || initial_capacity > ((size_t)1 << 40) ||
        (n_allow > 0 && (allow_bytes == nullptr || allow_offsets == nullptr))) {
        set_last_error("barcode_census_host: a null pointer with a size, or a size beyond its limit");
        return ROCCO_HIP_EINVAL;
    }
    const FragNames allow = {allow_bytes, allow_offsets, 0, (long long)n_allow};
    if (!barcode_census_host(bytes, n_bytes, allow, hash_mask, initial_capacity, bytes_out, bytes_capacity, offsets_out, records_out,
                             entries_capacity, report_out)) {
        set_last_error("barcode_census_host: the bytes hold " + std::to_string(report_out[0]) + " barcodes of " + std::to_string(report_out[1]) +
                       " bytes; offsets_out (one more than the entries) and records_out are both required and an output has room for fewer");
        return ROCCO_HIP_EINVAL;
    }
    return ROCCO_HIP_OK;
}

void rocco_hip_barcode_census_shape(int *shape_out)
{
    shape_out[0] = ROCCO_FRAGFILE_THREADS;
    shape_out[1] = ROCCO_FRAGFILE_THREADS;
    shape_out[2] = ROCCO_BARCODE_CENSUS_MAX_GRID;
    shape_out[3] = ROCCO_BARCODE_CENSUS_MIN_CAPACITY;
}

void rocco_hip_launch_caps(int *out)
{
    const int caps[] = {ROCCO_SELECT_GRID_TARGET,      ROCCO_SELECT_CHUNK_VALUES,     ROCCO_SELECT_THREADS,           ROCCO_BH_MAX_GRID,
                        ROCCO_BH_THREADS,              ROCCO_CHROM_RANGE_MAX_GRID,    ROCCO_COUNT_TAIL_MAX_GRID,      ROCCO_COUNT_THREADS,
                        ROCCO_INTERVAL_FACTS_MAX_GRID, ROCCO_COUNT_INTERVALS_THREADS, ROCCO_FRAGMENT_MAX_GRID,        ROCCO_FRAGMENT_THREADS,
                        ROCCO_FRAGMENT_DENSITY_RECORDS, ROCCO_FRAGMENT_DENSITY_WINDOW, ROCCO_BAM_MAX_GRID,            ROCCO_BAM_THREADS};
    static_assert(sizeof(caps) / sizeof(caps[0]) == ROCCO_LAUNCH_CAPS, "rocco_hip.h states the count");
    for (int k = 0; k < ROCCO_LAUNCH_CAPS; ++k) {
        out[k] = caps[k];
    }
}

int rocco_hip_synth_matrix(rocco_hip_solver *solver, void *matrix_dev, int dtype, size_t K, size_t n,
                           size_t row_stride, uint64_t seed, void *stream)
{
    if (solver == nullptr || matrix_dev == nullptr || row_stride < n || (dtype != 0 && dtype != 1)) {
        return ROCCO_HIP_EINVAL;
    }
    ROCCO_HIP_TRY(hipSetDevice(solver->device)); (void)hipGetLastError();  // (no other library's stale error for this call's launch checks)
    return launch_synth(matrix_dev, dtype, K, n, row_stride, seed, (hipStream_t)stream);
}

}  // extern "C"
