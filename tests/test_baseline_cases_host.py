"""tests/baseline_cases.py without a GPU: its sequential restatement of the cross-fit baseline is the oracle's bit for bit,
its forced plans are what the GPU tests mean them to be, and every "forced" / "met" label of a case is what `seam_meets`
finds at the case's seams -- so the GPU tests' assertions on the repair counter rest on something."""
import numpy as np
import pytest

import baseline_cases as bc


@pytest.mark.parametrize("window", bc.WINDOWS)
def test_restatement_is_the_oracle_bit_for_bit(oracle, window):
    lam = bc.penalty(window)
    rng = np.random.default_rng(window)
    for n in (25, 26, 27, 28, 63, 64, 65, 129, 1000, 4097, 5000):
        m = rng.normal(0.0, 3.0, size=(2, n)) * rng.choice([1.0, 100.0])
        m[1, :: 5] = 0.0
        m[1, 7] = -0.0
        assert bc.baseline_matrix(m, lam).tobytes() == oracle.crossfit_whittaker_baseline(m, lam).tobytes(), (window, n)
    assert bc.baseline_matrix(np.ones((2, 24)), lam).tobytes() == oracle.crossfit_whittaker_baseline(np.ones((2, 24)), lam).tobytes()


def test_restatement_on_the_adversarial_rows(oracle):
    """Signed zeros, denormals, huge and tiny values, a row that is not finite: same bits (NaNs: same places)."""
    for kind in bc.D4_KINDS + ("inf-in-row-3",):
        case = bc.d4_case(kind)
        m = case.matrix[:, :3000]
        got, want = bc.baseline_matrix(m, case.lam), oracle.crossfit_whittaker_baseline(m, case.lam)
        assert np.array_equal(np.isnan(got), np.isnan(want)), kind
        assert np.where(np.isnan(got), 0.0, got).tobytes() == np.where(np.isnan(want), 0.0, want).tobytes(), kind


def test_chain_states_are_the_sweeps_values():
    row = np.random.default_rng(1).normal(size=300)
    s = bc.RowSolve(row, bc.penalty(9))
    assert s.chain_state(0, "forward", 0) == (s.f[0][0], 0.0) and s.chain_state(1, "forward", 17) == (s.f[1][17], s.f[1][16])
    assert s.chain_state(1, "backward", 299) == (s.x[1][299], 0.0) and s.chain_state(0, "backward", 64) == (s.x[0][64], s.x[0][65])
    # a warm-up from the row's start (or end) is the row's own sweep; a short one at this penalty is not
    for sweep in ("forward", "backward"):
        for parity in (0, 1):
            assert bc.seam_meets(row, bc.penalty(9), parity, sweep, 128, 192)
            assert bc.seam_meets(s, bc.penalty(9), parity, sweep, 128, 1024)
    assert not bc.seam_meets(row, bc.penalty(101), 0, "forward", 192, 64)
    assert not bc.seam_meets(row, bc.penalty(101), 1, "backward", 64, 128)


def test_forced_plans_are_the_intended_ones():
    """Segments of 1 to 4 tiles, a last segment of one locus, warm-ups of 1 to 4 tiles -- longer than a segment, clipped at
    the row's end."""
    seen_tiles, one_locus_last, long_warm = set(), 0, 0
    for segment in bc.D1_SEGMENTS:
        for warm in bc.D1_WARMS:
            for cols in bc.d1_cols(segment):
                n_seg, seg_tiles, warm_tiles = bc.forced_plan(cols, segment, warm)
                assert n_seg >= 2 and 1 <= seg_tiles <= 4 and warm_tiles == warm // 64, (segment, warm, cols)
                seen_tiles.add(seg_tiles)
                one_locus_last += cols - (n_seg - 1) * seg_tiles * 64 == 1
                long_warm += warm_tiles > seg_tiles
    assert seen_tiles == {1, 2, 3, 4} and one_locus_last >= 3 and long_warm >= 10
    assert bc.forced_plan(2 * 64, 64, 64) == (2, 1, 1) and bc.forced_plan(2 * 64 + 1, 64, 64) == (2, 2, 1)
    assert bc.forced_plan(4 * 192 + 64, 192, 256) == (4, 4, 4) and bc.forced_plan(127, 64, 64)[0] == 1
    assert bc.forced_plan(bc.D2_COLS, bc.D2_SEGMENT, bc.D2_WARM) == (4, 17, 1)
    assert [bc.forced_plan(c, bc.D2_SEGMENT, bc.D2_WARM)[0] if c >= 25 else 0 for _r, c, _s in bc.D2_BATCH] == [s for _r, _c, s in bc.D2_BATCH]
    assert bc.forced_plan(bc.D3_SHAPE[1], bc.D3_SEGMENT, bc.D3_WARM) == (6, 65, 64)
    assert bc.forced_plan(bc.D4_COLS, bc.D4_SEGMENT, bc.D4_WARM) == (6, 33, 8)
    assert [bc.forced_plan(c, bc.D5_SEGMENT, bc.D5_WARM) for _r, c in bc.D5_SHAPES] == [(8, 17, 1), (8, 17, 1)]
    assert bc.D5_SHAPES[1][1] - 128 * 64 == 1  # (the last tile of the last segment holds one locus)


def _certify(case, forms=("baseline",), rows=None):
    assert case.label in ("forced", "met"), case
    assert len(case.seams()) >= 1, case
    for form in forms:
        if case.label == "forced":
            assert bc.open_seams(case, form, rows=rows, first_only=True), (case, form, "every seam meets")
        else:
            assert bc.open_seams(case, form, first_only=True) == [], (case, form)


@pytest.mark.parametrize("warm", bc.D1_WARMS)
@pytest.mark.parametrize("segment", bc.D1_SEGMENTS)
def test_small_tile_count_labels(segment, warm):
    cases = list(bc.d1_cases(segment, warm))
    assert len(cases) == 10
    for case in cases:
        _certify(case, ("baseline", "residual"))
    # what the label rests on: a warm-up that does not reach the row's end does not meet at this penalty -- at any seam
    for case in cases:
        if case.label == "forced" and case.rows == 1:
            n_seg, seg_tiles, warm_tiles = case.plan()
            tiles = -(-case.cols // 64)
            want = {(0, sweep, p, s * seg_tiles * 64) for s in range(1, n_seg) for p in (0, 1) for sweep in ("forward", "backward")
                    if (s * seg_tiles > warm_tiles if sweep == "forward" else s * seg_tiles + warm_tiles < tiles)}
            assert set(bc.open_seams(case)) == want, case
    assert {c.label for s in bc.D1_SEGMENTS for w in bc.D1_WARMS for c in bc.d1_cases(s, w)} == {"forced", "met"}


@pytest.mark.parametrize("rows", bc.D2_ROWS)
def test_second_wavefront_labels(rows):
    """... and the seam kernel's second workgroup has an open seam of its own: the last row of the 65- and 129-row cases."""
    _certify(bc.d2_case(rows), ("baseline", "residual"), rows=[rows - 1])


def test_mixed_batch_labels():
    batch = bc.d2_batch()
    assert [(c.rows, c.cols) for c in batch] == [(r, c) for r, c, _s in bc.D2_BATCH]
    for case in batch:
        if case.label is not None:
            _certify(case, ("baseline", "residual"), rows=[case.rows - 1])
        else:
            assert case.cols < 25 or case.plan()[0] == 1


@pytest.mark.parametrize("window", bc.WINDOWS)
def test_penalty_labels(window):
    _certify(bc.d3_case(window))


@pytest.mark.parametrize("kind", bc.D4_KINDS + ("inf-in-row-3",))
def test_adversarial_labels(kind):
    case = bc.d4_case(kind)
    _certify(case)
    seams = case.seams()
    if kind.startswith("spike"):
        # the true chains decay through ever smaller values behind the spike while a warm-up that starts behind it walks exact zeros
        for r in range(case.rows):
            (at,) = np.flatnonzero(case.matrix[r] >= 1e6)
            assert any(0 < s - at <= 4 for s in seams) and not case.matrix[r, at + 1:].any()
        assert {r for r, *_ in bc.open_seams(case)} == set(range(case.rows))
    if kind == "zeros-and-denormals":
        assert np.signbit(case.matrix[1]).all() and np.signbit(case.matrix[2, ::2]).all() and not case.matrix[:3].any()
        assert 0.0 < abs(case.matrix[3:7]).max() < 2.3e-308
    if kind == "inf-in-row-3":
        assert np.isfinite(np.delete(case.matrix, bc.D4_INF_ROW, axis=0)).all() and np.isinf(case.matrix[bc.D4_INF_ROW]).sum() == 1


@pytest.mark.parametrize("lam", bc.D5_PENALTIES)
def test_longer_factor_labels(lam):
    for case in bc.d5_cases(lam):
        _certify(case)
    assert bc.d5_long(lam).shape[1] > max(c for _r, c in bc.D5_SHAPES)
    assert lam not in [bc.penalty(w) for w in range(1, 1200)]
