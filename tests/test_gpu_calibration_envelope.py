"""GPU: the budgeted solve and the fixed-penalty solve at the edges of the fast path's numeric gates and of the target
(inputs and rules: tests/envelope_cases.py; the same rungs against search.cpp alone: tests/test_host_logic.py).

The gates are written down twice -- search.cpp (fast_path_applicable, analytic_count, bound_epsilon) for the host, the
director kernel of chain.hip for the device -- and outside them the sequential exact kernel (chain_exact.hip) answers
whole calibrations, bracket widening included.  Every case is compared with the oracle's sequential calibration
(rocco/dp.py:89-164 restated): penalty, count and solution bit for bit, the number of chain evaluations the reference
makes (62; 63 where it widens its bracket; 1 for target >= n), the penalised value by tests/tools/fuzz_parity.py's rule
(bit for bit where the exact kernel answered).  Which path answered is printed per case (run with -s), asserted only
where it is determined: the exact kernel outside the gates."""
import time

import numpy as np
import pytest

import envelope_cases as ec

pytestmark = pytest.mark.gpu

MODES = {  # (ROCCO_HIP_CHAIN, ROCCO_HIP_MODEL_CHAIN or None to leave it alone)
    "chain": ("1", None), "host": ("0", None), "chain-nomodel": ("1", "0"), "host-nomodel": ("0", "0")}
_ORACLE = {}  # the oracle's answers, shared between the modes of one case


def _set_mode(monkeypatch, mode):
    chain, model = MODES[mode]
    monkeypatch.setenv("ROCCO_HIP_CHAIN", chain)
    if model is None:
        monkeypatch.delenv("ROCCO_HIP_MODEL_CHAIN", raising=False)
    else:
        monkeypatch.setenv("ROCCO_HIP_MODEL_CHAIN", model)


def _reference(oracle, key, s, costs, target):
    if key not in _ORACLE:
        o_costs = oracle.build_switch_costs(s, costs) if np.isscalar(costs) else costs
        _ORACLE[key] = oracle.calibrate_selection_penalty(s, o_costs, target, return_evaluations=True)
    return _ORACLE[key]


def _check(got, ref, s, costs, where):
    """One calibration against the oracle's (penalty, solution, value, count, evaluations)."""
    pen, sol_t, val, cnt, info = got
    print("ENVELOPE", where, "path", info["path"], "evaluations", info["evaluations"], "count", cnt, "penalty", repr(pen))
    assert pen == ref[0], (where, pen, ref[0], info)
    assert cnt == ref[3], (where, cnt, ref[3], info)
    assert np.array_equal(sol_t.cpu().numpy(), ref[1]), (where, info)
    assert info["evaluations"] == ref[4], (where, info["evaluations"], ref[4], info)
    assert ec.values_agree(val, ref[2], ref[3], s, ref[0], info["path"] == 2), (where, val, ref[2], info)
    if s.size > 1 and not ec.inside_gates(s, costs):
        assert info["path"] == 2, (where, info)


def _calibrate(problems, stats=None):
    """problems: (scores, gamma or cost vector, target) each; ONE dp.calibrate_batch_device call."""
    import torch

    from rocco_amd import dp

    tensors = [torch.from_numpy(np.ascontiguousarray(s)).cuda() for s, _c, _t in problems]
    costs = [c if np.isscalar(c) else torch.from_numpy(c).cuda() for _s, c, _t in problems]
    return dp.calibrate_batch_device(tensors, costs, [t for _s, _c, t in problems], score_stats=stats)


# ---- a. the gate ladder, one gate at a time; c. under both sequencers ----------------------------------------------

def _ladder_params():
    for n in (33, 8191, 8193, 70000, 262145):
        for rung in ec.LADDER:
            for mode in MODES:
                if n >= 262145 or "nomodel" not in mode:
                    yield pytest.param(n, rung, mode, id="%d-%s-%s" % (n, rung, mode))


@pytest.mark.parametrize("n,rung,mode", list(_ladder_params()))
def test_gate_ladder(gpu, oracle, monkeypatch, n, rung, mode):
    _set_mode(monkeypatch, mode)
    for kind in ("peaks", "integers"):
        s, gamma = ec.rung_problem(rung, kind, n)
        for budget in ec.ladder_budgets(rung):
            target = int(np.floor(n * budget))
            ref = _reference(oracle, ("a", rung, kind, n, budget), s, gamma, target)
            if ec.widened(rung, n):
                assert ref[4] == 63, (rung, kind, n, budget, ref[4])
            t0 = time.perf_counter()
            got = _calibrate([(s, gamma, target)])[0]
            print("ENVELOPE seconds %.4f" % (time.perf_counter() - t0))
            _check(got, ref, s, gamma, ("ladder", rung, kind, n, budget, mode))


# ---- b. targets -----------------------------------------------------------------------------------------------------

def _target_params():
    for n in (2, 3, 8193, 300000):
        for kind in ("peaks", "integers", "normal"):
            for mode in MODES:
                if n >= 262145 or "nomodel" not in mode:
                    yield pytest.param(n, kind, mode, id="%d-%s-%s" % (n, kind, mode))


@pytest.mark.parametrize("n,kind,mode", list(_target_params()))
def test_targets_from_below_zero_to_past_the_end(gpu, oracle, monkeypatch, n, kind, mode):
    """Every target of one track in one batch (at n = 300000 the high budgets meet the compacted levels and the
    rounding-model chain); target >= n is one evaluation at penalty 0 (rocco/dp.py:102-108), target < 0 is target 0."""
    _set_mode(monkeypatch, mode)
    s = ec.track(kind, n)
    targets = ec.targets_for(n)
    refs = [_reference(oracle, ("b", kind, n, t), s, 1.0, t) for t in targets]
    for target, ref in zip(targets, refs):
        if target >= n:
            assert ref[4] == 1 and ref[0] == 0.0
    assert refs[0][0] == refs[1][0] and refs[0][4] == refs[1][4]  # -3 is 0
    out = _calibrate([(s, 1.0, t) for t in targets])
    for target, ref, got in zip(targets, refs, out):
        _check(got, ref, s, 1.0, ("targets", kind, n, target, mode))


# ---- d. one batch across every gate ---------------------------------------------------------------------------------

def _mixed_batch():
    rng = np.random.default_rng(20)
    normal = ec.track("normal", 30000)
    members = [
        ("ordinary", ec.track("peaks", 70000), 1.0, 1400),
        ("gamma just inside (1e-3)",) + ec.rung_problem("gamma=0.001", "integers", 8193) + (4096,),
        ("gamma just outside (9.99e-4)",) + ec.rung_problem("gamma=0.000999", "integers", 8193) + (4096,),
        ("gamma just inside (1e6)",) + ec.rung_problem("gamma=1000000.0", "peaks", 8191) + (163,),
        ("gamma just outside (1.000001e6)",) + ec.rung_problem("gamma=1000001.0", "peaks", 8191) + (163,),
        ("magnitude just inside (9e11)",) + ec.rung_problem("offset=900000000000.0", "peaks", 70000) + (35000,),
        ("magnitude just outside (1.1e12)",) + ec.rung_problem("offset=1100000000000.0", "peaks", 8193) + (4096,),
        ("spread just inside (1e9)",) + ec.rung_problem("spread=1000000000.0,gamma=1.0", "peaks", 70000) + (1400,),
        ("spread just outside (1.0000001e9)",) + ec.rung_problem("spread=1000000100.0,gamma=1.0", "peaks", 8193) + (163,),
        ("cost vector", normal, rng.uniform(0.5, 2.0, normal.size - 1), 600),
        ("target == n", ec.track("peaks", 8191), 1.0, 8191),
        ("63 evaluations (1e300)",) + ec.rung_problem("offset=1e+300", "integers", 8193) + (163,),
        ("63 evaluations (1e20)",) + ec.rung_problem("offset=1e+20", "peaks", 8193) + (4096,),
        ("one locus", np.array([0.7]), 1.0, 0),
    ]
    return members


@pytest.mark.parametrize("mode", ["chain", "host"])
def test_one_batch_across_every_gate(gpu, oracle, monkeypatch, mode):
    """One call holding an ordinary problem, one just inside and one just outside each gate, a cost vector, target == n,
    two problems on which the reference widens its bracket, and a single locus: every member gets its own
    single-problem oracle answer."""
    _set_mode(monkeypatch, mode)
    members = _mixed_batch()
    refs = [_reference(oracle, ("d", name), s, c, t) for name, s, c, t in members]
    assert refs[-3][4] == 63 and refs[-2][4] == 63 and refs[-4][4] == 1
    out = _calibrate([(s, c, t) for _name, s, c, t in members])
    for (name, s, c, _t), ref, got in zip(members, refs, out):
        _check(got, ref, s, c, ("mixed", name, mode))
    # n == 1: the library has no short cut (ROCCO_HIP_PATH_TRIVIAL is never reported); it runs the search on one locus
    assert out[-1][4]["path"] in (1, 2, 3, 4), out[-1][4]


@pytest.mark.parametrize("mode", ["chain", "host"])
def test_one_batch_across_every_gate_from_the_median_launch_statistics(gpu, oracle, monkeypatch, mode):
    """The same batch (without the cost vector: statistics are ignored for such a batch) solved from the min, max and
    sum |s| reduced inside the median launch.  Each matrix is three copies of the track, so the median is the track bit
    for bit (sum |s| of the 1e300 track is about 8e303 here: finite, and past every gate)."""
    import torch

    from rocco_amd import rocco as rr

    _set_mode(monkeypatch, mode)
    members = [m for m in _mixed_batch() if np.isscalar(m[2])]
    mats = [torch.from_numpy(np.ascontiguousarray(np.stack([s, s, s]))).cuda() for _name, s, _c, _t in members]
    scores, stats = rr.score_central_tendency_chrom_batch_device(mats, with_stats=True)
    assert stats is not None
    stats_h = stats.cpu().numpy()
    for (name, s, _c, _t), s_t, row in zip(members, scores, stats_h):
        assert np.array_equal(s_t.cpu().numpy(), s), name
        assert row[0] == s.min() and row[1] == s.max(), name
        assert np.isfinite(row[2]) and abs(row[2] - np.abs(s).sum()) <= 1e-12 * max(1.0, np.abs(s).sum()), name
    from rocco_amd import dp

    out = dp.calibrate_batch_device(scores, [c for _n, _s, c, _t in members], [t for _n, _s, _c, t in members],
                                    score_stats=stats_h)
    for (name, s, c, t), got in zip(members, out):
        _check(got, _reference(oracle, ("d", name), s, c, t), s, c, ("mixed+stats", name, mode))


# ---- e. fixed penalty -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rung", ec.MAGNITUDE_LADDER)
@pytest.mark.parametrize("n", [33, 8193, 70000])
def test_fixed_penalties_on_the_magnitude_rungs(gpu, oracle, n, rung):
    """dp.solve_penalized_chain at penalties below, above, inside and absurdly far from the scores, exactly on a score,
    and on / next to the penalty a calibration returns."""
    import torch

    from rocco_amd import dp

    for kind in ("peaks", "integers"):
        s, gamma = ec.rung_problem(rung, kind, n)
        costs = oracle.build_switch_costs(s, gamma)
        calibrated = _reference(oracle, ("e", rung, kind, n), s, gamma, int(np.floor(n * 0.02)))[0]
        s_t = torch.from_numpy(s).cuda()
        for lam in ec.fixed_penalties(s, calibrated):
            sol_t, val, cnt, path = dp.solve_penalized_chain_device(s_t, gamma, lam)
            o_sol, o_val, o_cnt = oracle.solve_penalized_chain(s, costs, lam)
            where = ("fixed", rung, kind, n, lam)
            print("ENVELOPE", where, "path", path, "count", cnt)
            assert cnt == o_cnt and np.array_equal(sol_t.cpu().numpy(), o_sol), (where, cnt, o_cnt, path)
            assert ec.values_agree(val, o_val, o_cnt, s, lam, path == 2), (where, val, o_val, path)
            if not ec.inside_gates(s, gamma):
                assert path == 2, (where, path)


# ---- f. a fixed-seed slice of what test_random_solves_fixed_seeds leaves out ---------------------------------------

def test_random_offset_solves_fixed_seeds(gpu, oracle):
    """100 random budgeted / fixed-penalty solves of the fuzzer's `offset` kind (scores far from zero, up to the magnitude
    gate), at budgets 0.5 and 0.9 and the switch costs at both ends of their gate."""
    import torch

    from rocco_amd import dp

    bad = []
    for it in range(100):
        rng = np.random.default_rng(888000 + it)
        n = int(rng.choice([1, 2, 3, 5, 31, 32, 33, 100, 1000, 8191, 8192, 8193, 20000, 70000, 300000]))
        offset = float(rng.choice([1e3, 3e4, -1e6, 1e9, 9e11]))
        s = offset + rng.gamma(1.0, 1.0, n)
        gamma = float(rng.choice([1e-3, 1e6]))
        costs = oracle.build_switch_costs(s, gamma)
        s_t = torch.from_numpy(s).cuda()
        if rng.random() < 0.6:
            target = int(np.floor(n * float(rng.choice([0.5, 0.9]))))
            g = dp.calibrate_selection_penalty_device(s_t, gamma, target)
            o = oracle.calibrate_selection_penalty(s, costs, target, return_evaluations=True)
            ok = (g[0] == o[0] and np.array_equal(g[1].cpu().numpy(), o[1]) and g[3] == o[3] and g[4]["evaluations"] == o[4]
                  and ec.values_agree(g[2], o[2], o[3], s, o[0], g[4]["path"] == 2))
            what = ("budget", target, g[4])
        else:
            lam = float(rng.choice([float(np.median(s)), offset + float(rng.normal()), float(np.max(s)) + 1.0, float(np.min(s)) - 1.0]))
            sol_t, val, cnt, path = dp.solve_penalized_chain_device(s_t, gamma, lam)
            o = oracle.solve_penalized_chain(s, costs, lam)
            ok = np.array_equal(sol_t.cpu().numpy(), o[0]) and cnt == o[2] and ec.values_agree(val, o[1], o[2], s, lam, path == 2)
            what = ("fixed", lam, path)
        print("ENVELOPE", ("slice", it, n, offset, gamma) + what, "ok" if ok else "MISMATCH")
        if not ok:
            bad.append((it, n, offset, gamma) + what)
    assert not bad, bad
