"""The product's host-side search / certification logic (rocco_amd/csrc/search.cpp, the very file
compiled into librocco_hip.so) driven on the CPU by an evaluator backed by the oracle
(tests/host_logic/harness.cpp).  Whatever path it takes, its answer must be the reference's:
solution and count bit-exact, penalty within 1e-9 (bit-exact when no decision was left open)."""
import os

import numpy as np
import pytest

import hostlogic as hl

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_vectors.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_golden_budget_cases(gold):
    for name in gold["bud_names"]:
        scores = gold[f"bud_{name}_scores"]
        budget, gamma = gold[f"bud_{name}_params"]
        target = int(np.floor(len(scores) * float(budget)))
        pen, sol, val, cnt, info = hl.calibrate(scores, float(gamma), target)
        pobj, count, frac, penalty = gold[f"bud_{name}_details"]
        assert np.array_equal(sol, gold[f"bud_{name}_solution"]), (name, info)
        assert cnt == int(count)
        assert abs(pen - penalty) <= 1e-9
        assert abs(val - pobj) <= 1e-9 * max(1.0, abs(pobj))
        assert info["evaluations"] == 62


def test_budget8_known_answer(gold):
    pen, sol, val, cnt, info = hl.calibrate(gold["budget8_scores"], 1.0, 3)
    assert sol.tolist() == [0, 0, 0, 0, 1, 1, 0, 0]
    assert pen == 1.05 and cnt == 2


@pytest.mark.parametrize("seed", range(8))
def test_random_problems_match_oracle(oracle, seed):
    from rocco_amd.synth import hash_matrix, survey_matrix

    rng = np.random.default_rng(seed)
    n = int(rng.choice([500, 5000, 40000]))
    K = int(rng.choice([1, 3, 10]))
    m = survey_matrix(n, K, 500 + seed) if seed % 2 == 0 else hash_matrix(K, n, seed=seed)
    s = np.median(m, axis=0) if K > 1 else m[0]
    budget = float(rng.choice([0.005, 0.02, 0.1]))
    gamma = float(rng.choice([0.5, 1.0, 10.0]))
    target = int(np.floor(n * budget))
    ref = oracle.calibrate_selection_penalty(s, oracle.build_switch_costs(s, gamma), target)
    for depth in (1, 3):
        pen, sol, val, cnt, info = hl.calibrate(s, gamma, target, spec_depth=depth)
        assert np.array_equal(sol, ref[1]), info
        assert cnt == ref[3]
        assert abs(pen - ref[0]) <= 1e-9
    # forcing the exact evaluator gives the reference bit for bit
    pen, sol, val, cnt, info = hl.calibrate(s, gamma, target, force_exact=True)
    assert (pen, val, cnt) == (ref[0], ref[2], ref[3]) and np.array_equal(sol, ref[1])
    assert info["path"] == 2


_DEVICE_SIDE_BEHAVIOURS = [
    {"NOW": "1"},                                                      # a compacted copy already exists: adopted at once
    {"NOW": "1", "SLACK": "1e-5", "TILE": "64"},                       # ... built at a lower penalty, tile borders kept
    {"POINTS": "64", "PILOT": "0.05", "TILE": "8192"},                 # 64 penalties a round, a good pilot
    {"POINTS": "7", "PILOT": "3.0", "PILOT_ROUNDS": "1", "PILOT_POINTS": "64"},  # a pilot that is wrong by 300 %
    {"COMPACT": "0"},                                                  # no compaction at all
]


@pytest.mark.parametrize("behaviour", range(len(_DEVICE_SIDE_BEHAVIOURS)))
def test_search_does_not_depend_on_what_the_device_side_does(oracle, monkeypatch, behaviour):
    """The evaluator of the harness imitates what the HIP evaluator may do behind the search's back -- adopt an
    existing compacted level (at once, built lower than asked, with tile borders kept), ask for few or many
    penalties a round, feed it pilot estimates of any quality -- and the answer must stay the reference's."""
    for key, value in _DEVICE_SIDE_BEHAVIOURS[behaviour].items():
        monkeypatch.setenv("ROCCO_HOSTLOGIC_" + key, value)
    kinds = ("round5", "int", "normal", "offset")
    for it in range(24):
        rng = np.random.default_rng([behaviour, it])
        n = int(rng.choice([33, 1000, 8193, 30000]))
        kind = kinds[it % len(kinds)]
        if kind == "round5":
            s = np.round(rng.gamma(1.0, 0.3, n), 5)
            s[rng.integers(0, n, max(1, n // 50))] += rng.gamma(6.0, 1.0, max(1, n // 50))
        elif kind == "int":
            s = rng.integers(-3, 6, n).astype(float)
        elif kind == "normal":
            s = rng.normal(0.2, 1.0, n)
        else:
            s = 1.0e3 + rng.gamma(1.0, 1.0, n)
        gamma = float(rng.choice([0.5, 1.0, 3.0]))
        target = int(np.floor(n * float(rng.choice([0.01, 0.05, 0.2]))))
        ref = oracle.calibrate_selection_penalty(s, oracle.build_switch_costs(s, gamma), target)
        pen, sol, val, cnt, info = hl.calibrate(s, gamma, target, spec_depth=1 + it % 3)
        assert pen == ref[0] and cnt == ref[3] and np.array_equal(sol, ref[1]), (kind, n, gamma, target, info)


def test_edge_cases_match_oracle(oracle):
    rng = np.random.default_rng(0)
    s = np.round(rng.gamma(1.0, 0.3, size=200), 5)
    for target in (0, 1, 199, 200, 1000):
        ref = oracle.calibrate_selection_penalty(s, oracle.build_switch_costs(s, 1.0), target)
        pen, sol, val, cnt, info = hl.calibrate(s, 1.0, target)
        assert np.array_equal(sol, ref[1]) and cnt == ref[3], (target, info)
        assert abs(pen - ref[0]) <= 1e-9
    # degenerate switch cost: the fast path must refuse and the exact evaluator answer
    ref = oracle.calibrate_selection_penalty(s, oracle.build_switch_costs(s, 0.0), 10)
    pen, sol, val, cnt, info = hl.calibrate(s, 0.0, 10)
    assert info["path"] == 2 and (pen, cnt) == (ref[0], ref[3]) and np.array_equal(sol, ref[1])
    # one locus
    ref = oracle.calibrate_selection_penalty(np.array([0.7]), np.zeros(0), 0)
    pen, sol, val, cnt, info = hl.calibrate(np.array([0.7]), 1.0, 0)
    assert np.array_equal(sol, ref[1]) and cnt == ref[3]


@pytest.mark.parametrize("offset,n,gamma,budget", [
    (1.0e3, 40000, 1.0, 0.05), (1.0e3, 3000, 1.0, 0.1), (3.0e4, 40000, 0.5, 0.1), (-1.0e6, 3000, 3.0, 0.05),
    (1.0e9, 100, 1.0, 0.3),
])
def test_scores_far_from_zero(oracle, offset, n, gamma, budget):
    """Scores whose magnitude dwarfs their spread: the reference adds the score BEFORE it subtracts the penalty
    (rocco/_chain_dp.c:120,125,127-128), so its roundings happen at the magnitude of the score, which the rounding
    model has to price whatever the running value is."""
    for seed in range(4):
        rng = np.random.default_rng([seed, n])
        s = offset + rng.gamma(1.0, 1.0, n)
        target = int(np.floor(n * budget))
        ref = oracle.calibrate_selection_penalty(s, oracle.build_switch_costs(s, gamma), target)
        pen, sol, val, cnt, info = hl.calibrate(s, gamma, target)
        assert pen == ref[0] and cnt == ref[3] and np.array_equal(sol, ref[1]), (seed, info)


def test_single_large_peak_at_the_end(oracle):
    """Target 0 on scores of magnitude 1e6: the penalty that stops selecting the last locus is decided by one
    rounding at that magnitude (a case the compacted copy of the chromosome once got wrong in the harness)."""
    bad = 0
    for it in range(300):
        rng = np.random.default_rng(it)
        n = int(rng.choice([5, 7, 12]))
        s = rng.normal(0, 1e6, n)
        gamma = float(rng.choice([0.5, 1.0, 3.0, 10.0, float(abs(rng.normal()) * 2)]))
        ref = oracle.calibrate_selection_penalty(s, oracle.build_switch_costs(s, gamma), 0)
        pen, sol, val, cnt, info = hl.calibrate(s, gamma, 0, spec_depth=1 + it % 3)
        bad += not (pen == ref[0] and cnt == ref[3] and np.array_equal(sol, ref[1]))
    assert bad == 0


def test_integer_scores_many_ties(oracle):
    """Integer data makes exact value ties the rule; whichever path is taken the answer is the
    reference's (count tie-break of rocco/_chain_dp.c:133-179)."""
    rng = np.random.default_rng(4)
    for _ in range(6):
        n = int(rng.integers(30, 3000))
        s = rng.integers(0, 6, size=n).astype(np.float64)
        target = int(n * 0.1)
        ref = oracle.calibrate_selection_penalty(s, oracle.build_switch_costs(s, 1.0), target)
        pen, sol, val, cnt, info = hl.calibrate(s, 1.0, target)
        assert np.array_equal(sol, ref[1]) and cnt == ref[3], info
        assert abs(pen - ref[0]) <= 1e-9


def test_fixed_penalty_matches_oracle(oracle):
    rng = np.random.default_rng(9)
    for _ in range(10):
        n = int(rng.integers(1, 5000))
        s = np.round(rng.gamma(1.0, 0.3, size=n), 5)
        gamma = float(rng.choice([0.5, 1.0, 3.0]))
        lam = float(rng.choice([-1.0, 0.0, 0.31, 2.0, 50.0]))
        sol, val, cnt, info = hl.solve_fixed(s, gamma, lam)
        o_sol, o_val, o_cnt = oracle.solve_penalized_chain(s, oracle.build_switch_costs(s, gamma), lam)
        assert np.array_equal(sol, o_sol) and cnt == o_cnt, (n, gamma, lam, info)
        assert abs(val - o_val) <= 1e-9 * max(1.0, abs(o_val))
    # vector costs
    n = 700
    s = np.round(rng.gamma(1.0, 0.3, size=n), 5)
    c = rng.uniform(0.2, 1.3, size=n - 1)
    sol, val, cnt, info = hl.solve_fixed(s, c, 0.4)
    o_sol, o_val, o_cnt = oracle.solve_penalized_chain(s, c, 0.4)
    assert np.array_equal(sol, o_sol) and cnt == o_cnt


def test_delta_definition_self_consistency(oracle):
    """The sequential delta-form definition agrees with the exact DP wherever it claims certainty:
    with no uncertain locus its fill equals the reference solution."""
    rng = np.random.default_rng(21)
    agree = 0
    for _ in range(30):
        n = int(rng.integers(10, 4000))
        s = np.round(rng.gamma(1.0, 0.3, size=n), 5)
        lam = float(rng.uniform(0.0, 1.0))
        sol, st = oracle.delta_chain(s, 1.0, lam)
        o_sol, _, o_cnt = oracle.solve_penalized_chain(s, oracle.build_switch_costs(s, 1.0), lam)
        if st["uncertain"] == 0 and not st["overflow"]:
            assert np.array_equal(sol, o_sol) and st["count"] == o_cnt
            agree += 1
        else:
            assert abs(st["count"] - o_cnt) <= st["effect"]
    assert agree >= 20


def test_host_logic_under_address_and_undefined_behaviour_sanitizers():
    """The product's search.cpp (1 400 lines of index-heavy host logic with prefetches ahead of the problem being planned) in
    ONE executable with the harness, the oracle's C sources and a driver, all compiled with -fsanitize=address,undefined
    (tests/host_logic/san_driver.cpp): 160 random calibrations + 320 fixed-penalty solves over six kinds of score arrays
    and eight imitated device-side behaviours, each compared with the oracle's sequential calibration, then the buffer
    layouts of test_model_chain_buffer_layouts (a fault there also makes the exit code 1).  Exit code 0 and an
    empty sanitizer log (CPU only: the pool has no GPU sanitizers)."""
    import os
    import subprocess

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_logic")
    subprocess.run(["make", "-C", here, "hostlogic_san"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([os.path.join(here, "hostlogic_san"), "160"], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "160 cases, 0 mismatches" in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr


def _check_layout_regions(regions, total, where):
    """`regions`: (name, offset, bytes it must hold) in the documented order.  Every region starts on a multiple of 256 where
    the one before ends, is as long as what it holds rounded up to 256 (so an empty one has length zero and none overlaps
    another), and the buffer ends with the last."""
    at = 0
    for k, (name, off, need) in enumerate(regions):
        end = regions[k + 1][1] if k + 1 < len(regions) else total
        assert off % 256 == 0, (where, name, off)
        assert off == at, (where, name, off, at)  # documented order, no gap, no overlap
        assert end - off == (need + 255) // 256 * 256, (where, name, off, end, need)
        if need == 0:
            assert end == off, (where, name)
        at = end
    assert at == total, (where, at, total)


def test_model_chain_buffer_layouts():
    """The device buffer, the pinned upload and the host-coherent buffer of a chain of rounding-model rounds
    (csrc/lean_tasks.h: model_chain_layout, the function csrc/budget.hip calls): an overlap of two scratch regions may still
    give right answers on small inputs, so the offsets are checked here, and at one shape against literal numbers."""
    lim = hl.model_chain_layout(1, 0, 1, 0)["limits"]
    assert lim["lean_max_points"] == 64
    shapes = [(1, 0, 1, 0), (1, 1, 3, 2048), (lim["chain_max_problems"], lim["chain_max_problems"], lim["model_chain_max_rounds"], 32768)]
    for B, n_wcap, rounds, cap_pairs in shapes:
        lay = hl.model_chain_layout(B, n_wcap, rounds, cap_pairs)
        where = (B, n_wcap, rounds, cap_pairs)
        _check_layout_regions(lay["device"], lay["device_bytes"], where)
        _check_layout_regions(lay["follow"], lay["follow_bytes"], where)
        # the upload is the device buffer's prefix [tasks][walk][wcap tasks]: it ends where `state` begins
        assert lay["upload_bytes"] == lay["device"][3][1], where
    first = hl.model_chain_layout(*shapes[0])
    sizes = {name: need for name, _off, need in first["device"]}
    assert sizes["wcap"] == 0 and sizes["entering"] == 0 and sizes["bits"] == 0
    # B = 1, one wcap task, 3 rounds, cap_pairs = 2048, by hand from the sums the evaluator used to spell out
    # (up(x) = x rounded up to 256; LeanTask and ModelChainWalk 144 bytes, LeanWcapTask 64, ModelChainState 88, LeanResult 24,
    # LeanWriteTask 48, ModelChainFinal 32, ModelChainFact 24, 64 penalties per problem and round):
    #   b_tasks = up(144) = 256, b_walk = up(144) = 256, b_wcap = up(64) = 256           -> up_bytes = 768
    #   state   at up_bytes = 768,                      b_state   = up(88)      = 256
    #   points  at 768 + 256 = 1024,                    b_points  = up(64 * 8)  = 512
    #   results at 1024 + 512 = 1536,                   b_results = up(64 * 24) = 1536
    #   ctl     at 1536 + 1536 = 3072, globals at ctl + 256 = 3328 (one 512-byte region)
    #   writes  at 3072 + 512 = 3584,                   b_writes  = up(48) = 256
    #   n_writes at 3584 + 256 = 3840 (a 256-byte slot)
    #   entering at 3840 + 256 = 4096,                  b_enter = up(3 * 2048 * 4) = 24576
    #   bits    at 4096 + 24576 = 28672,                b_bits  = 3 * 2048 * 2 * 256 * 4 = 12582912
    #   dev_bytes = 28672 + 12582912 = 12611584
    #   host-coherent: report at 0 (256 bytes), n_points at 256 with up(3 * 1 * 4) = 256, finals at 512 with up(32) = 256,
    #   facts at 768 with 3 * 1 * 64 * 24 = 4608 -> follow_bytes = 5376
    middle = hl.model_chain_layout(*shapes[1])
    assert [(name, off) for name, off, _need in middle["device"]] == [
        ("tasks", 0), ("walk", 256), ("wcap", 512), ("state", 768), ("points", 1024), ("results", 1536), ("ctl", 3072),
        ("globals", 3328), ("writes", 3584), ("n_writes", 3840), ("entering", 4096), ("bits", 28672)]
    assert middle["upload_bytes"] == 768 and middle["device_bytes"] == 12611584
    assert [(name, off) for name, off, _need in middle["follow"]] == [("report", 0), ("n_points", 256), ("finals", 512), ("facts", 768)]
    assert middle["follow_bytes"] == 5376


def test_record_launcher_scratch_layouts():
    """The scratch regions of the six record launchers (csrc/record_layouts.h: the structs count.hip, interval_count.hip and
    fragment_length.hip size their scratch with and take their pointers from): aligned, in order, without overlap, ending at
    the total, and every offset and total what the launchers computed before they shared `Layout` -- the sums of 256-rounded
    sizes their *_scratch_bytes and their pointer arithmetic spelt out, written out again here.  Shapes: around every size at
    which a rounding step changes ((T + 1) * 8 at T = 31 / 32, T * 4 at 64 / 65, pairs + 1 at 31 / 32 and 63 / 64, the 120
    bytes of a CountTrack between K = 2 and 3, the + 1 cell and the round-to-4 of a difference array, a scan tile of 2048
    bins, max_chunks + 1 cells at 63 / 64, hipcub temporary sizes around 0 and 256)."""
    up = lambda x: (x + 255) // 256 * 256
    tracks, blocks, pair_counts, temps = (1, 31, 32, 33, 64, 65), (1, 32, 33, 64, 65), (1, 31, 32, 63, 64, 65), (0, 1, 255, 256, 257)

    def check(kind, shape, sizes):
        regions, total = hl.record_layout(kind, *shape)
        _check_layout_regions(regions, total, (kind, shape))
        want, at = [], 0
        for size in sizes:
            want.append(at)
            at += up(size)
        assert [off for _name, off, _need in regions] == want and total == at, (kind, shape, regions, total, want, at)

    for K in (1, 2, 3):
        for bins in (1, 3, 4, 5, 2047, 2048, 2049):
            tiles, cells = K * ((bins + 2047) // 2048), K * ((bins + 1 + 3) // 4 * 4)
            check("count", (K, bins), [K * 120, (K + 1) * 4, (K + 1) * 4, K * 4, tiles * 4, cells * 4])
    for T in tracks:
        check("flag_facts", (T,), [(T + 1) * 8, T * 8, T * 4])
        for temp in temps:
            check("template", (T, temp), [(T + 1) * 8, T * 4, T * 4, max(temp, 1)])
            for pairs in pair_counts:
                check("interval", (T, pairs, temp), [(T + 1) * 8, 2 * T * 4, pairs * 8, pairs * 4, (pairs + 1) * 8, (pairs + 1) * 8, max(temp, 1)])
        for n in blocks:
            check("xcorr", (T, n), [(T + 1) * 8, T * 4, n * 4, n * 8, n * 4, n * 4, n * 4, n * 8])
    for max_chunks in (1, 63, 64):
        for temp in temps:
            check("centers", (max_chunks, temp), 6 * [(max_chunks + 1) * 4] + [max(temp, 1)])
    # K = 3 tracks of 2049 bins by hand: 360 bytes of tracks -> 512, 16 and 16 -> 256 each, maxima 12 -> 256, 6 tiles -> 256,
    # 3 * 2052 cells = 24624 bytes -> 24832: the buffer ends with the difference arrays, behind the maxima and the tile sums
    regions, total = hl.record_layout("count", 3, 2049)
    assert [(name, off) for name, off, _need in regions] == [
        ("tracks", 0), ("chunk_first", 512), ("tile_first", 768), ("maxima", 1024), ("tile_sums", 1280), ("delta", 1536)]
    assert total == 1536 + 24832


# ---- the envelope of the fast path's gates (inputs: tests/envelope_cases.py; the same rungs run on the GPU in
# tests/test_gpu_calibration_envelope.py, so a failure there can be placed: search.cpp here, the device side there) ----

def _calibrations_agree(oracle, s, gamma, target, where):
    import envelope_cases as ec

    ref = oracle.calibrate_selection_penalty(s, oracle.build_switch_costs(s, gamma), target, return_evaluations=True)
    pen, sol, val, cnt, info = hl.calibrate(s, gamma, target)
    assert pen == ref[0] and cnt == ref[3], (where, pen, ref[0], cnt, ref[3], info)
    assert np.array_equal(sol, ref[1]), (where, info)
    assert info["evaluations"] == ref[4], (where, info["evaluations"], ref[4], info)
    assert ec.values_agree(val, ref[2], ref[3], s, ref[0], info["path"] == 2, sequential=True), (where, val, ref[2], info)
    if s.size > 1 and not ec.inside_gates(s, gamma):
        assert info["path"] == 2, (where, info)
    return ref, info


@pytest.mark.parametrize("n", [33, 8191, 8193, 70000])
def test_envelope_gate_ladder(oracle, n):
    """One gate at a time, from just inside to far outside (switch cost, magnitude, spread), on the `peaks` and
    `integers` tracks at budgets 0.02 and 0.5: penalty, count, solution AND the number of chain evaluations are the
    reference's.  On the offsets +-1e20 (short tracks) and 1e300 the reference widens its bracket once: 63 evaluations."""
    import envelope_cases as ec

    widened = 0
    for rung in ec.LADDER:
        for kind in ("peaks", "integers"):
            s, gamma = ec.rung_problem(rung, kind, n)
            for budget in ec.ladder_budgets(rung):
                ref, _info = _calibrations_agree(oracle, s, gamma, int(np.floor(n * budget)), (rung, kind, n, budget))
                if ec.widened(rung, n):
                    assert ref[4] == 63, (rung, kind, n, budget, ref[4])
                    widened += 1
    assert widened == (3 if n <= 8193 else 1) * 2 * 2


@pytest.mark.parametrize("kind", ["peaks", "integers", "normal"])
@pytest.mark.parametrize("n", [2, 3, 8193, 70000])
def test_envelope_targets(oracle, kind, n):
    """Targets from below zero to past the end; target >= n is one evaluation at penalty 0 (rocco/dp.py:102-108)."""
    import envelope_cases as ec

    s = ec.track(kind, n)
    for target in ec.targets_for(n):
        ref, info = _calibrations_agree(oracle, s, 1.0, target, (kind, n, target))
        if target >= n:
            assert ref[4] == 1 and ref[0] == 0.0 and info["evaluations"] == 1


@pytest.mark.parametrize("n", [33, 8193, 70000])
def test_envelope_fixed_penalties(oracle, n):
    """solve_fixed on the magnitude rungs at penalties outside, inside and absurdly far from the scores, exactly on a
    score, and on / next to the calibrated penalty."""
    import envelope_cases as ec

    for rung in ec.MAGNITUDE_LADDER:
        for kind in ("peaks", "integers"):
            s, gamma = ec.rung_problem(rung, kind, n)
            costs = oracle.build_switch_costs(s, gamma)
            calibrated = oracle.calibrate_selection_penalty(s, costs, int(np.floor(n * 0.02)))[0]
            for lam in ec.fixed_penalties(s, calibrated):
                sol, val, cnt, info = hl.solve_fixed(s, gamma, lam)
                o_sol, o_val, o_cnt = oracle.solve_penalized_chain(s, costs, lam)
                assert np.array_equal(sol, o_sol) and cnt == o_cnt, (rung, kind, n, lam, info)
                assert ec.values_agree(val, o_val, o_cnt, s, lam, info["path"] == 2, sequential=True), (
                    rung, kind, n, lam, val, o_val, info)


# ---- off the reference's default of 60 bisection steps (inputs: tests/bisection_steps_cases.py; the same step counts
# run on the GPU in tests/test_gpu_calibration_steps.py, so a failure there can be placed: search.cpp here, the
# directors' replays and the chains there) ----

def _off_sixty_agree(oracle, kind, n, max_iter, where, depths=(1, 2, 3), exact=(False, True)):
    import bisection_steps_cases as bs
    import envelope_cases as ec

    s, gamma, target = bs.host_logic_problem(kind, n, 0)
    ref = bs.reference(oracle, ("host", kind, n), s, gamma, target, max_iter)
    assert ref[4] == max_iter + 2, (where, ref[4])
    for force_exact in exact:
        for depth in (depths[:1] if force_exact else depths):  # (the exact evaluator's trees have a depth of their own)
            pen, sol, val, cnt, info = hl.calibrate(s, gamma, target, max_iter=max_iter, spec_depth=depth, force_exact=force_exact)
            at = (where, kind, n, gamma, target, max_iter, depth, force_exact, info)
            assert pen == ref[0], (at, pen, ref[0])
            assert cnt == ref[3], (at, cnt, ref[3])
            assert np.array_equal(sol, ref[1]), at
            assert ec.values_agree(val, ref[2], ref[3], s, ref[0], info["path"] == 2, sequential=True), (at, val, ref[2])
            assert info["evaluations"] == max_iter + 2, at
            if force_exact:
                assert info["path"] == 2, at


def _step_counts():
    import bisection_steps_cases as bs

    return bs.STEP_COUNTS


@pytest.mark.parametrize("max_iter", _step_counts())
def test_calibration_off_sixty_steps(oracle, max_iter):
    """`max_iter` of rocco/dp.py:93 from 0 (the bracket's upper end is the answer) over a bisection cut in the middle of an
    open bracket to 200 (140 steps after the bracket stopped moving): four kinds of scores, four lengths, speculative
    depths 1 to 3, with and without the exact evaluator forced; penalty, count and solution are the reference's bit for
    bit and the evaluations are the reference's max_iter + 2."""
    for kind in ("round5", "int", "normal", "offset"):
        for n in (33, 1000, 8193, 30000):
            _off_sixty_agree(oracle, kind, n, max_iter, "plain")


@pytest.mark.parametrize("max_iter", [2, 26, 61, 120])
@pytest.mark.parametrize("behaviour", range(len(_DEVICE_SIDE_BEHAVIOURS)))
def test_off_sixty_steps_do_not_depend_on_what_the_device_side_does(oracle, monkeypatch, behaviour, max_iter):
    """The same check under every imitated device-side behaviour of
    test_search_does_not_depend_on_what_the_device_side_does."""
    import bisection_steps_cases as bs

    assert max_iter in bs.DEVICE_SIDE_STEP_COUNTS
    for key, value in _DEVICE_SIDE_BEHAVIOURS[behaviour].items():
        monkeypatch.setenv("ROCCO_HOSTLOGIC_" + key, value)
    for kind in ("round5", "int", "normal", "offset"):
        for n in (33, 1000, 8193, 30000):
            _off_sixty_agree(oracle, kind, n, max_iter, ("behaviour", behaviour))


def test_step_counts_span_every_regime(oracle):
    """The GPU tests lean on regimes that exist: on these tracks the ORACLE's own answers are far above every score
    (count 0) up to 17 steps, cut in the middle of an open bracket (a count that is not the one of 60 steps) below 60 and,
    on the integers, still at 59 and 61, differ from the penalty of 60 steps at 75 and 120, and have stopped moving by 75.
    The search itself is held to the same answers."""
    import bisection_steps_cases as bs
    import envelope_cases as ec

    seen = set()
    table = {}
    for kind, n, target, gamma in bs.REGIME_TRACKS:
        s = ec.track(kind, n)
        refs = {m: bs.reference(oracle, ("regime", kind, n, gamma), s, gamma, target, m) for m in bs.STEP_COUNTS + (60,)}
        table[kind] = (refs, bs.regimes(refs, target))
        for m, names in table[kind][1].items():
            seen |= {name for name in names if name != "past_sixty" or m > 60}
    assert seen == {"far", "cut_open", "past_sixty", "converged"}, seen
    refs, reg = table["normal"]
    assert all("far" in reg[m] for m in (0, 1, 2, 7, 17)), reg
    assert refs[0][0] > 262144.0 and refs[17][0] > 4.0, (refs[0][0], refs[17][0])  # max + sum(costs) + 1 halved 17 times
    assert all("past_sixty" in reg[m] for m in (75, 120, 200)) and "converged" in reg[75] and "converged" in reg[120], reg
    refs, reg = table["peaks"]
    assert all("cut_open" in reg[m] for m in (1, 2, 7, 17)) and not any("far" in reg[m] for m in (1, 2, 7, 17)), reg
    assert refs[7][3] < refs[17][3] < refs[26][3] == refs[60][3], [refs[m][3] for m in (7, 17, 26, 60)]
    assert all("past_sixty" in reg[m] for m in (75, 120, 200)) and "converged" in reg[75] and "converged" in reg[120], reg
    refs, reg = table["integers"]  # a count that still moves at 60
    assert "cut_open" in reg[59] and "cut_open" in reg[61] and refs[59][3] < refs[60][3] < refs[61][3], reg
    assert all("converged" in reg[m] for m in (61, 64, 65, 75, 120)), reg
    for kind, n, target, gamma in bs.REGIME_TRACKS:
        s = ec.track(kind, n)
        for m in (17, 61, 120):
            ref = table[kind][0][m]
            pen, sol, val, cnt, info = hl.calibrate(s, gamma, target, max_iter=m)
            assert pen == ref[0] and cnt == ref[3] and np.array_equal(sol, ref[1]), (kind, m, info)
            assert info["evaluations"] == m + 2 == ref[4], (kind, m, info)
