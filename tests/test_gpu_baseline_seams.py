"""GPU: the batched baseline sweeps (rocco_amd/csrc/whittaker.hip) where their rows are really cut -- segments of 1 to 4 tiles,
warm-ups longer than a segment, the seam kernel's second workgroup, slow and fast penalties, rows on which a warm-up
cannot meet the true chain, a cut row under a longer factor.  The cases, their forced plans and their "forced" / "met" labels
come from tests/baseline_cases.py (certified on the CPU by tests/test_baseline_cases_host.py).  Every case first asserts through
the library's plan query (rocco_hip_whittaker_batch_plan) that it is cut as intended; every comparison is bit for bit
against the oracle; the repair counter follows the case's label."""
import numpy as np
import pytest

import baseline_cases as bc

pytestmark = pytest.mark.gpu
FORMS = ("baseline", "residual")


def _seam_repairs():
    from rocco_amd import _native

    return int(_native.load().rocco_hip_whittaker_seam_repairs())


def _force(monkeypatch, segment, warm):
    monkeypatch.setenv("ROCCO_HIP_WHITTAKER_SEGMENT_LOCI", str(segment))
    monkeypatch.setenv("ROCCO_HIP_WHITTAKER_WARM_LOCI", str(warm))


def _assert_cut_as_intended(cases, form):
    """The library's plan of this very call against the cases' own: segments per row, tiles per segment, warm-up."""
    from rocco_amd import inference

    plan = inference.whittaker_batch_plan([(c.rows, c.cols) for c in cases], residual=(form == "residual"))
    want = [c.plan() if c.cols >= 25 else (0, 0, c.plan()[2]) for c in cases]
    assert plan["n_seg"] == [w[0] for w in want] and plan["seg_tiles"] == [w[1] for w in want], (cases, plan)
    assert plan["warm_tiles"] == want[0][2] and plan["budget_loci"] == 0, (cases, plan)
    for c, n_seg in zip(cases, plan["n_seg"]):
        assert (n_seg >= 2) == (c.label is not None), (c, plan)
    if any(n >= 2 for n in plan["n_seg"]):
        assert plan["grouped"], plan
        assert plan["workgroups"] == sum(-(-c.rows // 16) * n for c, n in zip(cases, plan["n_seg"])), (cases, plan)
    return plan


def _want(oracle, case, form):
    if form == "baseline":
        return oracle.crossfit_whittaker_baseline(case.matrix, case.lam)
    g = case.sweep_input("residual")
    return g - oracle.crossfit_whittaker_baseline(g, case.lam)


def _run(gpu, cases, form):
    """One call of the batch entry of `form` on the cases' matrices; (outputs as arrays, repairs counted by the call)."""
    import torch
    from rocco_amd import inference

    lam = cases[0].lam
    mats = [torch.from_numpy(c.matrix).to(gpu) for c in cases]
    before = _seam_repairs()
    if form == "baseline":
        outs = inference.crossfit_whittaker_baseline_batch_device(mats, lam)
    else:
        offs = [None if c.offsets is None else torch.from_numpy(c.offsets).to(gpu) for c in cases]
        outs = inference.crossfit_whittaker_residual_batch_device(mats, offs, lam)
    repairs = _seam_repairs() - before
    for m, c in zip(mats, cases):
        assert m.cpu().numpy().tobytes() == c.matrix.tobytes(), (c, "the input was written to")
    return [o.cpu().numpy() for o in outs], repairs


def _check(gpu, oracle, cases, form, wants=None):
    _assert_cut_as_intended(cases, form)
    outs, repairs = _run(gpu, cases, form)
    for k, (c, o) in enumerate(zip(cases, outs)):
        want = _want(oracle, c, form) if wants is None else wants[k]
        assert o.tobytes() == want.tobytes(), (c, form, int((o.view(np.int64) != want.view(np.int64)).sum()), "values differ")
    labels = {c.label for c in cases} - {None}
    if "forced" in labels:
        assert repairs > 0, (cases, form, "no seam was recomputed")
    elif labels == {"met"}:
        assert repairs == 0, (cases, form, repairs, "seams were recomputed")
    return repairs


def test_plan_query_says_what_the_launcher_does(gpu, monkeypatch, capfd):
    """rocco_hip_whittaker_batch_plan against the launcher's own account of a launch (ROCCO_HIP_WHITTAKER_TRACE on stderr): the
    budget, the workgroups and the matrices cut, at forced and at default settings; the lone whole matrix takes the per-row
    sweep in the baseline form only; the query launches nothing."""
    import re

    import torch
    from rocco_amd import inference

    def traced(shapes):
        mats = [torch.zeros(s, dtype=torch.float64, device=gpu) for s in shapes]
        capfd.readouterr()
        inference.crossfit_whittaker_baseline_batch_device(mats, bc.penalty(101))
        found = re.findall(r"\[whittaker\] (\d+) matrices: a workgroup walks <= (\d+) loci, warm-up (\d+), (\d+) workgroups of <= \d+ rows "
                           r"\((\d+) resident\), (\d+) matrices cut", capfd.readouterr().err)
        assert len(found) == 1, found
        return [int(v) for v in found[0]]

    monkeypatch.setenv("ROCCO_HIP_WHITTAKER_TRACE", "1")
    default_warm = inference.whittaker_batch_plan([(1, 100)])["warm_tiles"] * 64
    for settings in ((bc.D2_SEGMENT, bc.D2_WARM), None):
        if settings is not None:
            _force(monkeypatch, *settings)
            shapes = [(r, c) for r, c, _s in bc.D2_BATCH]
        else:
            monkeypatch.delenv("ROCCO_HIP_WHITTAKER_SEGMENT_LOCI")
            monkeypatch.delenv("ROCCO_HIP_WHITTAKER_WARM_LOCI")
            shapes = [(2, 2 * default_warm + 200), (17, 5000), (1, 24)]
        before = _seam_repairs()
        plan = inference.whittaker_batch_plan(shapes)
        assert _seam_repairs() == before
        count, budget, warm, workgroups, _resident, n_cut = traced(shapes)
        assert (count, budget, workgroups, n_cut) == (len(shapes), plan["budget_loci"], plan["workgroups"], sum(n >= 2 for n in plan["n_seg"])), plan
        assert -(-warm // 64) == plan["warm_tiles"] and plan["grouped"] and n_cut >= 1
    lone = inference.whittaker_batch_plan([(3, 5000)])
    assert lone["n_seg"] == [1] and not lone["grouped"] and lone["workgroups"] == 3, lone
    assert inference.whittaker_batch_plan([(3, 5000)], residual=True)["grouped"]
    assert inference.whittaker_batch_plan([(3, 5000)], with_offsets=True)["grouped"]
    both = inference.whittaker_batch_plan([(3, 5000), (40, 24), (0, 100), (33, 64)])
    assert both["n_seg"] == [1, 0, 0, 1] and both["grouped"] and both["workgroups"] == 1 + 3, both
    monkeypatch.setenv("ROCCO_HIP_WHITTAKER_SEGMENT_LOCI", "0")
    assert inference.whittaker_batch_plan([(2, 3 * default_warm)])["n_seg"] == [1]


# ---- D1 ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("warm", bc.D1_WARMS)
@pytest.mark.parametrize("segment", bc.D1_SEGMENTS)
def test_segments_of_one_to_four_tiles(gpu, oracle, monkeypatch, segment, warm):
    """Rows of 2 S to 5 S - 1 loci in segments of 1 to 4 tiles, a last segment of one locus, warm-ups of 1 to 4 tiles that
    reach over several predecessors or are clipped at the row's end; 1 row and 17 (two groups), both forms.  A warm-up this
    short meets nothing at the penalty of window 101: the counter rises wherever some warm-up is not the row's own sweep
    from its end, and stays where every one is."""
    _force(monkeypatch, segment, warm)
    cases = list(bc.d1_cases(segment, warm))
    assert len(cases) == 10 and {c.rows for c in cases} == {1, 17}
    for case in cases:
        want = {form: _want(oracle, case, form) for form in FORMS}
        for form in FORMS:
            _check(gpu, oracle, [case], form, [want[form]])


# ---- D2 ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", bc.D2_ROWS)
def test_seams_of_rows_past_the_first_wavefront(gpu, oracle, monkeypatch, rows):
    """63, 64, 65 and 129 rows: the seam kernel's lanes all busy, one row and one lane of a second and third workgroup, with
    open seams in every row."""
    _force(monkeypatch, bc.D2_SEGMENT, bc.D2_WARM)
    case = bc.d2_case(rows)
    for form in FORMS:
        repairs = _check(gpu, oracle, [case], form)
        # every row has open seams (64 loci of warm-up): far more than the first 64 rows could account for is not claimed,
        # but each row's first forward seam alone makes `rows` of them
        assert repairs >= rows, (rows, form, repairs)


def test_cut_uncut_short_and_grouped_matrices_in_one_batch(gpu, oracle, monkeypatch):
    """A cut 65-row matrix, an uncut one, one too short for a baseline, a cut one of another segment count and a cut one of
    two row groups (9 + 8) in ONE pair of launches: the seam records, the task bases and the states of each are its own."""
    _force(monkeypatch, bc.D2_SEGMENT, bc.D2_WARM)
    cases = bc.d2_batch()
    for form in FORMS:
        plan = _assert_cut_as_intended(cases, form)
        assert plan["n_seg"] == [4, 1, 0, 2, 3]
        _check(gpu, oracle, cases, form)


# ---- D3 ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", bc.WINDOWS)
def test_penalties_that_contract_faster_and_slower(gpu, oracle, monkeypatch, window):
    """Windows 3 and 9 (a warm-up of 4096 loci meets), 101 and 1001 (it does not): the bits are the oracle's either way and
    the counter follows what tests/test_baseline_cases_host.py found for the case."""
    _force(monkeypatch, bc.D3_SEGMENT, bc.D3_WARM)
    case = bc.d3_case(window)
    assert case.label == ("met" if window < 100 else "forced")  # (stated here too: a relabelled case must be looked at)
    for form in FORMS:
        _check(gpu, oracle, [case], form)


def test_window_1001_at_default_settings(gpu, oracle, monkeypatch):
    """The slowest penalty at the DEFAULT plan, on rows the plan cuts in two: the oracle's bits.  Whether 196 608 loci of
    warm-up meet at this penalty is reported, not asserted (DESIGN.md section 13.2 measured the count path's penalty only)."""
    import torch
    from rocco_amd import inference

    monkeypatch.delenv("ROCCO_HIP_WHITTAKER_SEGMENT_LOCI", raising=False)
    monkeypatch.delenv("ROCCO_HIP_WHITTAKER_WARM_LOCI", raising=False)
    warm = inference.whittaker_batch_plan([(2, 1000)])["warm_tiles"] * 64
    cols = bc.first_length(lambda c: inference.whittaker_batch_plan([(2, c)])["n_seg"][0] >= 2, 2 * warm, 3 * warm)
    plan = inference.whittaker_batch_plan([(2, cols)])
    assert plan["n_seg"] == [2] and plan["grouped"] and plan["workgroups"] == 2, plan
    lam = bc.penalty(1001)
    h = np.random.default_rng(1001).normal(0.0, 2.0, size=(2, cols))
    before = _seam_repairs()
    out = inference.crossfit_whittaker_baseline_batch_device([torch.from_numpy(h).to(gpu)], lam)[0]
    print(f"window 1001, default plan {plan}, {cols} loci: {_seam_repairs() - before} seams recomputed")
    assert out.cpu().numpy().tobytes() == oracle.crossfit_whittaker_baseline(h, lam).tobytes()


# ---- D4 ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", bc.D4_KINDS)
def test_rows_on_which_chains_do_not_meet(gpu, oracle, monkeypatch, kind):
    """A spike before a seam and exact zeros behind it (the true chain decays through ever smaller values, the warm-up's is
    exactly zero), a step at a seam, constant and zero rows side by side, zeros of both signs and denormals, blocks of
    1e-290 and 1e200: the oracle's bytes -- signs of zeros included -- in both forms."""
    _force(monkeypatch, bc.D4_SEGMENT, bc.D4_WARM)
    case = bc.d4_case(kind)
    for form in FORMS:
        _check(gpu, oracle, [case], form)


def test_a_row_that_is_not_finite_beside_finite_ones(gpu, oracle, monkeypatch):
    """+inf in row 3 only: the other rows keep the oracle's bits, row 3 is NaN exactly where the oracle's is and equal
    elsewhere (a NaN's sign and payload are left free); the residual form refuses the matrix as the reference does."""
    import torch
    from rocco_amd import inference

    _force(monkeypatch, bc.D4_SEGMENT, bc.D4_WARM)
    case = bc.d4_case("inf-in-row-3")
    _assert_cut_as_intended([case], "baseline")
    with np.errstate(all="ignore"):
        want = oracle.crossfit_whittaker_baseline(case.matrix, case.lam)
    (out,), repairs = _run(gpu, [case], "baseline")
    others = [r for r in range(case.rows) if r != bc.D4_INF_ROW]
    assert out[others].tobytes() == want[others].tobytes()
    got3, want3 = out[bc.D4_INF_ROW], want[bc.D4_INF_ROW]
    assert np.isnan(want3).any()
    assert np.array_equal(np.isnan(got3), np.isnan(want3))
    assert got3[~np.isnan(want3)].tobytes() == want3[~np.isnan(want3)].tobytes()
    assert repairs > 0
    _assert_cut_as_intended([case], "residual")
    with pytest.raises(ValueError, match="non-finite"):
        inference.crossfit_whittaker_residual_batch_device([torch.from_numpy(case.matrix).to(gpu)], None, case.lam)


# ---- D5 ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("on_device", [0, 1])
def test_cut_rows_under_a_longer_factor(gpu, oracle, monkeypatch, on_device):
    """The device's factor of a penalty is the longest row's; a shorter row takes its last entries from
    whittaker_tail_kernel's recomputation.  A 40 001-locus matrix first, then cut rows of 8 200 and 8 193 loci (the last
    segment ends in a tile of 8 loci / of one locus) whose last segments and seam repairs read those entries; the factor
    walked by the host threads and by the device's own kernel."""
    import torch
    from rocco_amd import inference

    _force(monkeypatch, bc.D5_SEGMENT, bc.D5_WARM)
    monkeypatch.setenv("ROCCO_HIP_FACTOR_ON_DEVICE", str(on_device))
    lam = bc.D5_PENALTIES[on_device]
    long_h = bc.d5_long(lam)
    out = inference.crossfit_whittaker_baseline_batch_device([torch.from_numpy(long_h).to(gpu)], lam)[0]
    assert out.cpu().numpy().tobytes() == oracle.crossfit_whittaker_baseline(long_h, lam).tobytes()
    cases = bc.d5_cases(lam)
    for form in FORMS:
        _check(gpu, oracle, cases, form)
    _check(gpu, oracle, cases[1:], "baseline")  # (the lone matrix: cut, so the grouped kernels and not the per-row sweep)
