"""GPU: the calibration off the reference's default of 60 bisection steps, on every solve path (inputs and regimes:
tests/bisection_steps_cases.py; the same step counts against search.cpp alone: tests/test_host_logic.py).

`max_iter` (rocco/dp.py:93,141) is replayed by search.cpp on the host and twice by the director of the rounding-model
chain on the device (model_chain.hip: plan_round and the walk that follows a round); the threshold chain of chain.hip
does not know it.  budget.hip sizes the model chain from it (at most 16 rounds) and takes a solution the chain wrote
only when no step was left.  Every case is compared with the oracle's sequential calibration at the same `max_iter`: penalty,
count and solution bit for bit, the reference's max_iter + 2 chain evaluations, the penalised value by
tests/envelope_cases.py's rule.  Path, passes, zone_iters and the model chain's counters are printed per case (-s)."""
import ctypes

import numpy as np
import pytest

import bisection_steps_cases as bs
import envelope_cases as ec

pytestmark = pytest.mark.gpu


def _model_chain_counters():
    from rocco_amd import _native

    out = (ctypes.c_longlong * 4)()
    _native.load().rocco_hip_model_chain_counters(out)
    return list(out)  # chains, counts taken over, counts answered from them, counts asked for that a chain had not evaluated


def _written_counters():
    from rocco_amd import _native

    out = (ctypes.c_longlong * 2)()
    _native.load().rocco_hip_model_chain_written_counters(out)
    return list(out)  # solutions the chains wrote themselves, final windows answered from them


def _calibrate(problems, max_iter):
    """problems: (scores, gamma or cost vector, target) each; ONE dp.calibrate_batch_device call."""
    import torch

    from rocco_amd import dp

    tensors = [torch.from_numpy(np.ascontiguousarray(s)).cuda() for s, _c, _t in problems]
    costs = [c if np.isscalar(c) else torch.from_numpy(c).cuda() for _s, c, _t in problems]
    return dp.calibrate_batch_device(tensors, costs, [t for _s, _c, t in problems], max_iter=max_iter)


def _check(got, ref, s, where, evaluations):
    """One calibration against the oracle's (penalty, solution, value, count, evaluations)."""
    pen, sol_t, val, cnt, info = got
    print("STEPS", where, "n", len(s), "path", info["path"], "passes", info["passes"], "zone_iters", info["zone_iters"],
          "n_diff", info["n_diff"], "maps", info["maps"], "count", cnt, "penalty", repr(pen))
    assert pen == ref[0], (where, pen, ref[0], info)
    assert cnt == ref[3], (where, cnt, ref[3], info)
    assert np.array_equal(sol_t.cpu().numpy(), ref[1]), (where, info)
    assert ec.values_agree(val, ref[2], ref[3], s, ref[0], info["path"] == 2), (where, val, ref[2], info)
    assert ref[4] == evaluations and info["evaluations"] == evaluations, (where, info["evaluations"], ref[4], evaluations)


# the one (kind, max_iter, ROCCO_HIP_CHAIN) at 45 steps and more where no rounding-model chain starts on the compacted batch: a
# chain is wanted only in a round whose every request is a rounding-model probe with two rounds or more ahead (budget.hip:
# model_chain_wanted), and at 45 steps on `peaks` the host-sequenced search has no such round left (the device-sequenced
# one, whose problems arrive together, has)
NO_CHAIN_STARTS = {("peaks", 45, "0")}


def _chains_engaged(before, after, started, where):
    """The model chain's counters over the calibrations of ONE sequencer: chains started and counts answered from them
    (tests/test_gpu_chain.py holds both at 60), or -- the named exception -- none, and nothing asked for in vain."""
    if started:
        assert after[0] > before[0] and after[2] > before[2], (where, before, after)
    else:
        assert after[0] == before[0], (where, before, after)
    assert after[3] == before[3], (where, before, after)


def _references(oracle, name, problems, max_iter):
    return [bs.reference(oracle, (name, k), s, c, t, max_iter) for k, (s, c, t) in enumerate(problems)]


def _solve_and_check(monkeypatch, problems, refs, max_iter, where, chains=("1", "0")):
    for chain in chains:
        monkeypatch.setenv("ROCCO_HIP_CHAIN", chain)
        out = _calibrate(problems, max_iter)
        for (s, _c, _t), ref, got in zip(problems, refs, out):
            _check(got, ref, s, where + ("chain=" + chain,), max_iter + 2)


# ---- a. every step count against the oracle -------------------------------------------------------------------------

@pytest.mark.parametrize("max_iter", bs.STEP_COUNTS)
@pytest.mark.parametrize("kind", bs.KINDS)
def test_every_step_count_gives_the_oracles_calibration(gpu, oracle, monkeypatch, kind, max_iter):
    """tests/test_gpu_chain.py's batch (8191 to 262145 loci, n = 2 and 3) with the threshold search sequenced by the
    device and by the host."""
    problems = bs.batch(kind)
    refs = _references(oracle, ("a", kind), problems, max_iter)
    _solve_and_check(monkeypatch, problems, refs, max_iter, ("a", kind, max_iter))


# ---- b. the rounding-model chain off 60 -----------------------------------------------------------------------------

@pytest.mark.parametrize("model_chain,follow", [("1", "1"), ("1", "0"), ("0", "1"), ("0", "0")])
@pytest.mark.parametrize("max_iter", bs.COMPACTED_STEP_COUNTS)
@pytest.mark.parametrize("kind", bs.COMPACTED_KINDS)
def test_rounding_model_chain_off_sixty_steps(gpu, oracle, monkeypatch, kind, max_iter, model_chain, follow):
    """A batch whose every problem ends on a compacted level, so that the rounding-model rounds run as a chain whose
    director replays what is left of `max_iter`.  With the model chain allowed, under EACH sequencer chains start from 45
    steps on (but for NO_CHAIN_STARTS, where none must) and every count the host's replay asks for is among the counts the
    chain evaluated (tests/test_gpu_chain.py holds both at 60)."""
    monkeypatch.setenv("ROCCO_HIP_MODEL_CHAIN", model_chain)
    monkeypatch.setenv("ROCCO_HIP_CHAIN_FOLLOW", follow)
    problems = bs.compacted_batch(kind)
    refs = _references(oracle, ("b", kind), problems, max_iter)
    for chain in ("1", "0"):
        before = _model_chain_counters()
        _solve_and_check(monkeypatch, problems, refs, max_iter, ("b", kind, max_iter, model_chain, follow), chains=(chain,))
        after = _model_chain_counters()
        print("STEPS model chain counters", (kind, max_iter, model_chain, follow, chain), [a - b for a, b in zip(after, before)])
        if model_chain == "0":
            assert after == before, (before, after)
        elif max_iter >= 45:
            _chains_engaged(before, after, (kind, max_iter, chain) not in NO_CHAIN_STARTS, (kind, max_iter, chain))
        else:
            assert after[3] == before[3], (kind, max_iter, chain, before, after)


@pytest.mark.parametrize("max_iter", bs.COMPACTED_STEP_COUNTS)
@pytest.mark.parametrize("kind", bs.COMPACTED_KINDS)
def test_solutions_written_by_the_chain_off_sixty_steps(gpu, oracle, monkeypatch, kind, max_iter):
    """The chain writes the final solution itself only when no step is left at its end: the oracle's solutions whether it
    may (ROCCO_HIP_CHAIN_WRITE=1) or not, and with =0 nothing counted as written.  At 59 and 61 steps the chains walk the
    bisection to its last step and write; from 75 steps on the steps behind the last chain belong to the zone / spine
    endgame (path 4), so no chain ends with no step left and none may count a solution as written."""
    problems = bs.compacted_batch(kind)
    refs = _references(oracle, ("b", kind), problems, max_iter)
    for write in ("1", "0"):
        monkeypatch.setenv("ROCCO_HIP_CHAIN_WRITE", write)
        before = _written_counters()
        _solve_and_check(monkeypatch, problems, refs, max_iter, ("b-write", kind, max_iter, write))
        after = _written_counters()
        print("STEPS written counters", (kind, max_iter, write), [a - b for a, b in zip(after, before)])
        if write == "0":
            assert after == before, (before, after)
        else:
            assert 0 <= after[1] - before[1] <= after[0] - before[0], (before, after)  # windows answered from written solutions
            if max_iter in (59, 61):
                assert after[0] > before[0], (kind, max_iter, before, after)
            if max_iter >= 75:
                assert after == before, (kind, max_iter, before, after)


# ---- c. chains that end with steps left -----------------------------------------------------------------------------

@pytest.mark.parametrize("rounds", ["1", "2", "3"])
@pytest.mark.parametrize("variable", ["ROCCO_HIP_MODEL_CHAIN_ROUNDS", "ROCCO_HIP_CHAIN_ROUNDS"])
@pytest.mark.parametrize("max_iter", [60, 120])
@pytest.mark.parametrize("kind", bs.COMPACTED_KINDS)
def test_chains_that_end_with_steps_left(gpu, oracle, monkeypatch, kind, max_iter, variable, rounds):
    """A rounding-model chain (or the threshold chain before it) cut after one to three rounds hands a bisection with
    steps still open back to the host, which must finish it from the chain's facts: nothing may be taken as written."""
    monkeypatch.setenv(variable, rounds)
    for name, problems in (("c", bs.compacted_batch(kind)), ("a", bs.batch(kind))):
        if name == "a" and variable != "ROCCO_HIP_CHAIN_ROUNDS":
            continue  # (the short problems meet the threshold chain only)
        refs = _references(oracle, (name, kind) if name == "a" else ("b", kind), problems, max_iter)
        for chain in ("1", "0"):
            before = _model_chain_counters()
            _solve_and_check(monkeypatch, problems, refs, max_iter, ("c", name, kind, max_iter, variable, rounds), chains=(chain,))
            after = _model_chain_counters()
            print("STEPS model chain counters", (name, kind, max_iter, variable, rounds, chain), [a - b for a, b in zip(after, before)])
            if name == "c":
                _chains_engaged(before, after, True, (kind, max_iter, variable, rounds, chain))


@pytest.mark.parametrize("kind", bs.COMPACTED_KINDS)
def test_the_sixteen_round_clamp_at_two_hundred_steps(gpu, oracle, monkeypatch, kind):
    """200 steps ask for more rounds than a chain holds (budget.hip clamps at kModelChainMaxRounds = 16)."""
    monkeypatch.delenv("ROCCO_HIP_MODEL_CHAIN_ROUNDS", raising=False)
    monkeypatch.delenv("ROCCO_HIP_CHAIN_ROUNDS", raising=False)
    problems = bs.compacted_batch(kind)
    refs = _references(oracle, ("b", kind), problems, 200)
    for chain in ("1", "0"):
        before = _model_chain_counters()
        _solve_and_check(monkeypatch, problems, refs, 200, ("c-clamp", kind), chains=(chain,))
        after = _model_chain_counters()
        print("STEPS model chain counters", ("clamp", kind, chain), [a - b for a, b in zip(after, before)])
        _chains_engaged(before, after, True, ("clamp", kind, chain))


# ---- d. one batch, a step count per problem -------------------------------------------------------------------------

def _mixed_steps_batch():
    rng = np.random.default_rng(31)
    normal = ec.track("normal", 30000)
    # (8191, 8193, 70000, 3, 2, 262145 loci: the counts past 60 on the long problems, neighbours never alike)
    members = [(s, c, t, m) for (s, c, t), m in zip(bs.batch("peaks"), (60, 61, 120, 7, 0, 200))]
    members += [
        (normal, rng.uniform(0.5, 2.0, normal.size - 1), 600, 33),  # a cost vector: the host's machinery
        (np.array([0.7]), 1.0, 0, 5),                               # one locus
        (ec.track("peaks", 8191), 1.0, 8191, 45),                   # target == n: 0.0 before any bisection
        (ec.track("integers", 8193), 1.0, 0, 26),                   # target 0
        (ec.track("normal", 120_000), 1.0, 2400, 75),               # ends on a compacted level, past 60
    ]
    return members


@pytest.mark.parametrize("chain", ["1", "0"])
def test_one_batch_with_a_step_count_per_problem(gpu, oracle, monkeypatch, chain):
    """The task of the C ABI carries its own max_iter: one call mixing 0 to 200 steps, a cost vector, one locus,
    target == n (the reference returns 0.0 after ONE evaluation whatever max_iter is) and target 0, each member against
    its own oracle call; three calls on one solver give the same answers (no shared scratch left dirty)."""
    monkeypatch.setenv("ROCCO_HIP_CHAIN", chain)
    members = _mixed_steps_batch()
    problems = [(s, c, t) for s, c, t, _m in members]
    steps = [m for _s, _c, _t, m in members]
    refs = [bs.reference(oracle, ("d", k), s, c, t, m) for k, (s, c, t, m) in enumerate(members)]
    assert refs[8][0] == 0.0 and refs[8][4] == 1, refs[8]
    for rep in range(3):
        out = _calibrate(problems, steps)
        for k, ((s, _c, _t, m), ref, got) in enumerate(zip(members, refs, out)):
            _check(got, ref, s, ("d", k, m, "chain=" + chain, rep), 1 if k == 8 else m + 2)
    with pytest.raises(ValueError):
        _calibrate(problems, steps[:-1])  # one step count per problem, or one for all


# ---- e. the single-problem wrappers ---------------------------------------------------------------------------------

@pytest.mark.parametrize("max_iter", [0, 5, 61])
def test_single_problem_wrappers_take_max_iter(gpu, oracle, max_iter):
    """dp.calibrate_selection_penalty on host arrays (the reference's signature, rocco/dp.py:89-94: a cost VECTOR) and
    calibrate_selection_penalty_device with the scalar switch cost."""
    import torch

    from rocco_amd import dp

    s = ec.track("peaks", 70000)
    costs = oracle.build_switch_costs(s, 1.0)
    ref = bs.reference(oracle, ("e",), s, 1.0, 1400, max_iter)
    pen, sol, val, cnt = dp.calibrate_selection_penalty(s, costs, 1400, max_iter=max_iter)
    assert isinstance(sol, np.ndarray) and sol.dtype == np.uint8
    assert pen == ref[0] and cnt == ref[3] and np.array_equal(sol, ref[1]), (max_iter, pen, ref[0], cnt, ref[3])
    assert ec.values_agree(val, ref[2], ref[3], s, ref[0], False), (val, ref[2])
    got = dp.calibrate_selection_penalty_device(torch.from_numpy(s).cuda(), 1.0, 1400, max_iter=max_iter)
    _check(got, ref, s, ("e", max_iter), max_iter + 2)


# ---- a negative max_iter ----------------------------------------------------------------------------------------------

def test_negative_max_iter_is_no_step_in_python_and_refused_by_the_c_abi(gpu, oracle):
    """The reference's `for _ in range(max_iter)` takes no step for a negative count (rocco/dp.py:141); the Python forms
    do the same, the C ABI answers ROCCO_HIP_EINVAL (include/rocco_hip.h) and leaves the results alone."""
    import torch

    from rocco_amd import _native, dp

    s = ec.track("peaks", 8193)
    costs = oracle.build_switch_costs(s, 1.0)
    ref = oracle.calibrate_selection_penalty(s, costs, 163, max_iter=-3, return_evaluations=True)
    zero = bs.reference(oracle, ("negative",), s, 1.0, 163, 0)
    assert ref[0] == zero[0] and ref[4] == 2 and np.array_equal(ref[1], zero[1])
    pen, sol, _val, cnt = dp.calibrate_selection_penalty(s, costs, 163, max_iter=-3)
    assert pen == ref[0] and cnt == ref[3] and np.array_equal(sol, ref[1])
    s_t = torch.from_numpy(s).cuda()
    _check(dp.calibrate_selection_penalty_device(s_t, 1.0, 163, max_iter=-1), ref, s, ("negative", "device"), 2)
    out = dp.calibrate_batch_device([s_t, s_t], [1.0, 1.0], [163, 163], max_iter=[-7, 0])
    for got in out:
        _check(got, ref, s, ("negative", "batch"), 2)
    # the C ABI
    lib = _native.load()
    solver = _native.solver_for(s_t.device.index)
    sol_t = torch.zeros(s.size, dtype=torch.uint8, device=s_t.device)
    tasks = (_native.BudgetTask * 1)()
    results = (_native.BudgetResult * 1)()
    tasks[0].scores_dev = s_t.data_ptr()
    tasks[0].switch_costs_dev = None
    tasks[0].gamma = 1.0
    tasks[0].n = s.size
    tasks[0].target_count = 163
    tasks[0].sum_costs = float(np.sum(costs))
    tasks[0].max_iter = -1
    tasks[0].solution_dev = sol_t.data_ptr()
    results[0].evaluations = -77
    stream = int(torch.cuda.current_stream().cuda_stream)
    assert lib.rocco_hip_solve_budget_batch_f64(solver.handle, 1, tasks, results, stream) == _native.EINVAL
    assert lib.rocco_hip_solve_budget_batch_stats_f64(solver.handle, 1, tasks, None, results, stream) == _native.EINVAL
    assert results[0].evaluations == -77 and int(sol_t.sum().item()) == 0
    tasks[0].max_iter = 0
    assert lib.rocco_hip_solve_budget_batch_f64(solver.handle, 1, tasks, results, stream) == _native.OK
    torch.cuda.synchronize()
    assert results[0].selection_penalty == ref[0] and results[0].evaluations == 2
    assert np.array_equal(sol_t.cpu().numpy(), ref[1])
