"""GPU: objective_value (rocco_amd/csrc/objective.hip, rocco/dp.py:16-34) at the edges of its summation tree, against
the exact value and within an ABSOLUTE bound derived from the tree -- not relative to the result, which says nothing where
gain and switch penalty cancel.

Reference.  With z in {0, 1} every product s[i] * z[i] and c[i] * |z[i+1] - z[i]| is a term itself or zero, so the true
value is -sum(s[z != 0]) + sum(c[dz != 0]).  The tests take the kernel's error without a rounding of their own:
math.fsum over the kernel's result, the selected scores and the negated switch costs is the correctly rounded difference
between the result and that true value.

Bound.  Gain and penalty are summed by the same tree, separately.  The additions on the longest path a term can take:
    8                     the lane's serial loop over its 8 loci (objective_partial_kernel; the first adds to 0.0)
    6                     shuffle steps of block_sum (offsets 32 .. 1)
    4                     wavefront sums added serially by lane 0 of block_sum (256 lanes = 4 wavefronts; the first adds to 0.0)
    ceil(tiles / 256)     the serial loop `t += kThreads` of objective_final_kernel over tile partials (tile = 2048 loci)
    6 + 4                 its block_sum
    1                     the last -g + p
that is D = 29 + ceil(tiles / 256).  The products round nothing (one factor is 0 or 1; a fused multiply-add rounds once, as
the addition it replaces does).  Each addition multiplies what it carries by (1 + d), |d| <= u = 2^-53, so a term t ends up
as t * prod(1 + d_j) over at most D factors and the error is at most ((1 + u)^D - 1) * sum|t|.  At least three of the D
additions add to 0.0 and are exact, and (1 + u)^(D - 3) - 1 <= D * u for every D below 2^25, so

    |result - true| <= D * 2^-53 * (sum |s[i]| z[i] + sum c[i] |dz[i]|).

The batch kernels walk the same tree task by task; calibrate_batch_device's penalized value is checked against
objective_value of its own solution, see test_batch_tree_matches_single_launch."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LANE_LOCI = 8
TILE = 256 * LANE_LOCI
FINAL_LANES = 256
U = 2.0 ** -53
SIZES = (1, 2, 7, 8, 9, 2047, 2048, 2049, 4097, FINAL_LANES * TILE - 1, FINAL_LANES * TILE, FINAL_LANES * TILE + 1,
         2 * FINAL_LANES * TILE + 2049)
LAST_COST = 1.0e6
INPUTS = ("random", "ones", "alt10", "only_last", "cancel", "mixed")


def additions_on_longest_path(n):
    tiles = -(-n // TILE)
    return 8 + 6 + 4 + -(-tiles // FINAL_LANES) + 6 + 4 + 1


def test_path_length_restated():
    assert additions_on_longest_path(1) == additions_on_longest_path(FINAL_LANES * TILE) == 30
    assert additions_on_longest_path(FINAL_LANES * TILE + 1) == 31 and additions_on_longest_path(SIZES[-1]) == 32
    for d in (30, 31, 32, 1 << 20):
        assert (1.0 + 2.0 ** -52) ** (d - 3) - 1.0 <= d * 2.0 ** -52  # (the inequality of the docstring, at twice the unit)


def _costs(n, kind):
    """gamma, or a cost vector of length n - 1 whose last entry is large: reading cs[n - 1] or skipping cs[n - 2] shows."""
    if kind == "scalar":
        return 1.75
    c = np.random.default_rng(500 + n).uniform(0.5, 2.0, size=max(n - 1, 0))
    if n >= 2:
        c[-1] = LAST_COST
    return c


def _problem(n, kind, costs):
    """(z uint8, scores float64) of one input kind."""
    rng = np.random.default_rng(31 * n + INPUTS.index(kind))
    s = rng.standard_normal(n) * 3.0 + 1.0
    z = (rng.random(n) < 0.35).astype(np.uint8)
    if kind == "ones":
        z[:] = 1
    elif kind == "alt10":
        z[:] = 0
        z[::2] = 1
    elif kind == "only_last":
        z[:] = 0
        z[-1] = 1
    elif kind == "mixed":
        s = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-8.0, 8.0, size=n)
    elif kind == "cancel":
        # gain == switch penalty to within 1e-12 of either: the result is rounding noise of sums of size `penalty`
        s = rng.uniform(0.5, 2.0, size=n)
        if n >= 2:
            z[:2] = [1, 0]  # at least one selected locus and one switch
        penalty = _penalty_terms(z, costs)
        gain = math.fsum(s[z != 0].tolist())
        if penalty.size and gain > 0.0:
            s = s * (math.fsum(penalty.tolist()) / gain)
    return z, s


def _penalty_terms(z, costs):
    switches = np.flatnonzero(np.diff((z != 0).astype(np.int8)) != 0)
    if np.isscalar(costs):
        return np.full(switches.size, float(costs))
    return np.asarray(costs)[switches]


def _error_and_bound(got, z, s, costs):
    """(got - true value, correctly rounded;  the derived bound;  -fsum(gains) + fsum(penalties), for the printed line)."""
    gains = s[z != 0]
    pens = _penalty_terms(z, costs)
    err = math.fsum([got] + gains.tolist() + (-pens).tolist())
    magnitude = math.fsum(np.abs(gains).tolist()) + math.fsum(np.abs(pens).tolist())
    want = -math.fsum(gains.tolist()) + math.fsum(pens.tolist())
    return err, additions_on_longest_path(z.shape[0]) * U * magnitude, want


@pytest.mark.parametrize("cost_kind", ["scalar", "vector"])
@pytest.mark.parametrize("n", SIZES)
def test_objective_within_derived_bound(gpu, n, cost_kind):
    import torch
    from rocco_amd import dp

    costs = _costs(n, cost_kind)
    costs_arg = costs if cost_kind == "scalar" else torch.from_numpy(costs).to(gpu)
    for kind in INPUTS:
        z, s = _problem(n, kind, costs)
        z_t, s_t = torch.from_numpy(z).to(gpu), torch.from_numpy(s).to(gpu)
        got = dp.objective_value(z_t, s_t, costs_arg)
        err, bound, want = _error_and_bound(got, z, s, costs)
        print(f"n={n} {cost_kind} {kind}: got={got!r} want={want!r} err={err:.3e} bound={bound:.3e}")
        assert abs(err) <= bound, (n, cost_kind, kind, got, want, err, bound)
        assert dp.objective_value(z_t, s_t, costs_arg) == got, (n, cost_kind, kind)  # run to run: bit-equal
        if kind == "ones":
            assert _penalty_terms(z, costs).size == 0
        if kind == "only_last" and n >= 2:
            assert math.fsum(_penalty_terms(z, costs).tolist()) == (LAST_COST if cost_kind == "vector" else costs)
        if kind == "alt10":
            assert _penalty_terms(z, costs).size == n - 1
        if kind == "cancel" and n >= 7:
            pen = math.fsum(_penalty_terms(z, costs).tolist())
            assert pen > 0.0 and abs(math.fsum(s[z != 0].tolist()) - pen) <= 1e-12 * pen


@pytest.mark.parametrize("cost_kind", ["scalar", "vector"])
@pytest.mark.parametrize("n", [9, 2049, FINAL_LANES * TILE + 1])
def test_non_zero_bytes_are_selected(gpu, n, cost_kind):
    import torch
    from rocco_amd import dp

    costs = _costs(n, cost_kind)
    costs_arg = costs if cost_kind == "scalar" else torch.from_numpy(costs).to(gpu)
    z, s = _problem(n, "random", costs)
    z[-1] = 1
    s_t = torch.from_numpy(s).to(gpu)
    want = dp.objective_value(torch.from_numpy(z).to(gpu), s_t, costs_arg)
    assert want != 0.0
    mix = np.where(z != 0, np.random.default_rng(n).choice(np.array([1, 2, 0x80, 0xFF], dtype=np.uint8), size=n), 0).astype(np.uint8)
    for other in (z * 255, z * 2, z * 0x80, mix):
        other = other.astype(np.uint8)
        assert np.array_equal(other != 0, z != 0) and other.max() > 1
        assert dp.objective_value(torch.from_numpy(other).to(gpu), s_t, costs_arg) == want


BATCH_LENGTHS = [2049, FINAL_LANES * TILE + 1, 2047, FINAL_LANES * TILE, 4097]  # both sides of a tile, both sides of 256 tiles


def _batch_problems(gpu, cost_kind):
    import torch

    assert BATCH_LENGTHS.index(max(BATCH_LENGTHS)) != 0
    scores, costs, targets = [], [], []
    for i, n in enumerate(BATCH_LENGTHS):
        rng = np.random.default_rng(900 + i)
        s = rng.standard_normal(n) + 3.0 * (rng.random(n) < 0.05)
        scores.append(torch.from_numpy(s).to(gpu))
        costs.append(0.5 + 0.25 * i if cost_kind == "scalar" else torch.from_numpy(rng.uniform(0.25, 1.5, size=n - 1)).to(gpu))
        targets.append(int(0.03 * n))
    return scores, costs, targets


@pytest.mark.parametrize("cost_kind", ["vector", "scalar"])
def test_batch_tree_matches_single_launch(gpu, monkeypatch, cost_kind):
    """calibrate_batch_device's penalized value is `-objective - penalty * count` with the objective from
    objective_partial_batch_kernel / objective_final_batch_kernel.  Recomputed with objective_value on the solution it
    returned, the two may differ only by what a fused multiply-add in the host expression (budget.hip, `penalized_values`)
    could change: one rounding of the product and one of the result.  A batch kernel that mapped a tile to the wrong task or
    dropped a partial would miss by many orders of magnitude more.

    "The same tree" is a statement about the same arrays.  With a cost vector the solve never restricts a problem to a
    compacted level (`lean_eligible`: costs == nullptr), so the batch kernels read the caller's arrays.  With a scalar gamma
    they may read the compacted level instead -- fewer loci, other tile seams, another rounding -- so that form runs here
    with ROCCO_HIP_LEAN=0 (read per call); the default path is test_batch_value_on_compacted_levels_within_derived_bound."""
    from rocco_amd import dp

    if cost_kind == "scalar":
        monkeypatch.setenv("ROCCO_HIP_LEAN", "0")
    scores, costs, targets = _batch_problems(gpu, cost_kind)
    out = dp.calibrate_batch_device(scores, costs, targets)
    assert len(out) == len(BATCH_LENGTHS)
    for i, (penalty, sol_t, value, count, _info) in enumerate(out):
        assert int(sol_t.sum().item()) == count and 0 < count <= targets[i], i
        obj = dp.objective_value(sol_t, scores[i], costs[i])
        want = -obj - penalty * count
        allowed = float(np.spacing(abs(penalty * count)) + np.spacing(abs(value)))
        print(f"task {i} n={BATCH_LENGTHS[i]} {cost_kind}: value={value!r} recomputed={want!r} diff={value - want:.3e} allowed={allowed:.3e}")
        assert abs(value - want) <= allowed, (i, BATCH_LENGTHS[i], value, want, allowed)


def test_batch_value_on_compacted_levels_within_derived_bound(gpu):
    """Scalar gamma on the default path: the objective behind the penalized value may have been summed over a compacted
    level (on an MI355X: task 3, n = 524 288, value 7422.827359297677 against 7422.827359297669 from objective_value on
    the caller's arrays, 8 units in the last place; bit-equal with ROCCO_HIP_LEAN=0).  A compacted level holds a subset
    of the loci with every selected locus and every switch among them, in no more tiles, so the bound of the module
    docstring for the full length covers it; the host expression adds the rounding of penalty * count and of the result."""
    from rocco_amd import dp

    scores, costs, targets = _batch_problems(gpu, "scalar")
    out = dp.calibrate_batch_device(scores, costs, targets)
    for i, (penalty, sol_t, value, count, _info) in enumerate(out):
        assert int(sol_t.sum().item()) == count and 0 < count <= targets[i], i
        z, s = sol_t.cpu().numpy(), scores[i].cpu().numpy()
        gains, pens = s[z != 0], _penalty_terms(z, costs[i])
        err = math.fsum([value, penalty * count] + (-gains).tolist() + pens.tolist())  # value - (gain - switches - penalty * count)
        tree = additions_on_longest_path(BATCH_LENGTHS[i]) * U * (math.fsum(np.abs(gains).tolist()) + math.fsum(pens.tolist()))
        allowed = tree + float(np.spacing(abs(penalty * count)) + np.spacing(abs(value)))
        print(f"task {i} n={BATCH_LENGTHS[i]} default path: value={value!r} err={err:.3e} allowed={allowed:.3e}")
        assert abs(err) <= allowed, (i, BATCH_LENGTHS[i], value, err, allowed)
