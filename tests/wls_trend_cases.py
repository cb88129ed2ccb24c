"""Cases for the y side of the sort-free trend fit (rocco_amd/csrc/wls.hip: wls_deal_kernel, seg_select_*,
seg_gather_kernel, seg_settle_kernel, seg_select_finish_kernel, wls_knots_rows_kernel), built on DICTATED local variances:
`score_centered_wls_device(..., variances_t=V)` takes each row's rolling variances from the caller, so a case decides which
multiset of y every trend bin holds.

A case is (m [K, n], V [K, n - window + 1], kwargs, expected wls_sorted_rows(), claims).  The builder knows every locus's bin
from argsort(|x|) (bin b: sorted ranks [b n // bins, (b + 1) n // bins)), gives the bins the values the case needs, writes
V[c] = y[c + half] and then RECOMPUTES what the scoring will see, y'[i] = max(V[clamp(i - half, 0, n - window)], 1e-8): the
`half` loci at each end of a row read a neighbour's variance.  Every claim is made on y' (`census`), never on the values the
builder meant to place; the edge loci of a crafted row are moved into bins the case does not craft (their x is exchanged with
an inner locus's, which leaves the multiset of |x| and so the bins' ranks as they were).

Terms: key(y) = the bit pattern of the positive double y; a CELL = key >> 42, the 22 bits known after the first two counting
passes (digits: bits 63..53, 52..42, then 41..31, 30..20, 19..9, 8..0); a bin's MEDIAN CELL COUNT = how many of its y' share
the cell of its lower median (sorted rank (w - 1) // 2).  Cells of at most CELL_MAX values are gathered and sorted in LDS
(padded to a power of two, at least 64); larger ones take the four remaining passes and the "above" pass.

tests/test_wls_trend_cases_host.py checks the claims on the CPU; tests/test_gpu_wls_trend_edges.py runs the cases."""
import functools
import math

import numpy as np

CELL_MAX = 4096       # kCellMax
SELECT_CHUNK = 8192   # kSelectChunk
SELECT_MIN = 4096     # kTrendSelectMin: shorter rows sort their pairs
BASE = 1.5e-3         # the crafted cells' smallest value
FLOOR = 1.0e-8
FLOORED_INPUTS = (0.0, -0.0, 5e-324, 1e-300, 9.99e-9, 1.0e-8)  # all 1e-8 behind the floor


def trend_bins(n):
    """wls_backend.c:461, the expression of `trend_bins` in rocco_amd/csrc/wls.hip."""
    return int(max(4, math.floor(1 + math.log(n + 1) / math.log(2))))


def bin_edges(n, bins=None):
    bins = trend_bins(n) if bins is None else bins
    return [(b * n) // bins for b in range(bins + 1)]


def even_bins(n):
    e = bin_edges(n)
    return [b for b in range(len(e) - 1) if (e[b + 1] - e[b]) % 2 == 0]


def keys(y):
    return np.ascontiguousarray(y, dtype=np.float64).view(np.uint64)


def cells(y):
    return keys(y) >> np.uint64(42)


def in_cell(j):
    """Distinct values of BASE's cell: BASE (1 + j 2^-40)."""
    return BASE * (1.0 + np.asarray(j, dtype=np.float64) * 2.0 ** -40)


def seen_variances(V, n, window):
    """y': what the scoring reads for every locus (wls_backend.c:727-738, then the floor of 429-430)."""
    half = window // 2
    c = np.clip(np.arange(n) - half, 0, n - window)
    return np.maximum(V[:, c], FLOOR)


def padded(count):
    """LDS slots seg_settle_kernel sorts for a cell of `count` values."""
    p = 64
    while p < count:
        p <<= 1
    return p


def census(x_row, y_row, b, bins=None):
    """The structure of bin b of one row, from |x| and y' alone (pairs ordered by (x, y) as the reference orders them)."""
    n = x_row.shape[0]
    e = bin_edges(n, bins)
    order = np.lexsort((y_row, np.abs(x_row)))
    seg = np.sort(y_row[order[e[b]:e[b + 1]]])
    w = seg.shape[0]
    r0 = (w - 1) // 2
    lower, upper = seg[r0], seg[w // 2]
    cs, ks = cells(seg), keys(seg)
    mine = cs == cs[r0]
    eq = np.flatnonzero(seg == lower)
    return {
        "width": w, "even": w % 2 == 0, "rank": r0, "lower": float(lower), "upper": float(upper),
        "cell_count": int(mine.sum()), "cell_distinct": bool(np.unique(seg[mine]).size == int(mine.sum())),
        "rank_in_cell": int(r0 - np.flatnonzero(mine)[0]),
        "padded": padded(int(mine.sum())),
        "run_first": int(eq[0]), "run_last": int(eq[-1]), "run": int(eq.size), "count_le": int(eq[-1]) + 1,
        "lower_is_cell_max": bool(lower == seg[mine].max()), "lower_is_cell_min": bool(lower == seg[mine].min()),
        "upper_in_cell": bool(cs[w // 2] == cs[r0]), "upper_far": bool(upper >= 2.0 ** 10 * lower),
        "first_digits": int(np.unique(ks >> np.uint64(53)).size), "cells": int(np.unique(cs).size),
        "shared_high_bits": next(s for s in range(65) if s == 64 or np.unique(ks >> np.uint64(s)).size == 1),
        "distinct": int(np.unique(seg).size), "chunks": -(-w // SELECT_CHUNK),
    }


def bin_medians(x_row, y_row):
    n = x_row.shape[0]
    e = bin_edges(n)
    ys = y_row[np.lexsort((y_row, np.abs(x_row)))]
    return np.array([np.median(ys[e[b]:e[b + 1]]) for b in range(len(e) - 1)])


# ---- what a bin is given: functions (width, rng) -> width values ------------------------------------------------------------------

def _below(rng, k):
    return 1.0e-6 * (1.0 + rng.random(k))   # cells far below BASE's


def _above(rng, k):
    return 2.0 * (1.0 + rng.random(k))      # cells far above: more than 2^10 times BASE


def craft_cell(count, pos):
    """`count` distinct values of one cell, the bin's lower median the one of rank `pos` among them; the rest of the bin far
    below and far above."""
    def make(w, rng):
        lo = (w - 1) // 2 - pos
        hi = w - lo - count
        assert lo >= 0 and hi >= 0, (w, count, pos)
        return np.concatenate([_below(rng, lo), in_cell(np.arange(count)), _above(rng, hi)])
    return make


def craft_run(length, past, same_cell_above):
    """A run of `length` values equal to BASE that ends at sorted rank (w - 1) // 2 + past, then `same_cell_above` distinct
    values of its cell, then values far above; far below before the run."""
    def make(w, rng):
        lo = (w - 1) // 2 + past - length + 1
        hi = w - lo - length - same_cell_above
        assert lo >= 0 and hi >= 0, (w, length, past)
        return np.concatenate([_below(rng, lo), np.full(length, BASE), in_cell(1 + np.arange(same_cell_above)), _above(rng, hi)])
    return make


def craft_floored(past):
    """Given variances at or below the floor, mixed, as many as make their run of 1e-8 end at rank (w - 1) // 2 + past; then
    three times the next double above the floor, then plain values."""
    def make(w, rng):
        f = (w - 1) // 2 + past + 1
        low = np.array([FLOORED_INPUTS[i % len(FLOORED_INPUTS)] for i in range(f)])
        return np.concatenate([low, np.full(3, np.nextafter(FLOOR, 1.0)), _plain(rng, w - f - 3)])
    return make


def craft_low_bits(w, rng):
    """Consecutive bit patterns: digits 1-4 agree, the fifth takes a few values, the last all 512."""
    first = (keys(np.array([BASE]))[0] >> np.uint64(20)) << np.uint64(20)
    return (first + np.arange(w, dtype=np.uint64)).view(np.float64)


def craft_full_range(w, rng):
    v = 10.0 ** np.linspace(-8.0, 300.0, w)
    v[0], v[-1] = FLOOR, 1.0e300
    return v


def _plain(rng, shape):
    return 0.5 * np.exp(rng.normal(0.0, 0.7, size=shape))  # spread out the way variances are


# ---- the builder ------------------------------------------------------------------------------------------------------------------

def _matrix(rng, K, n):
    m = rng.normal(0.0, 1.0, size=(K, n))
    for k in range(K):
        assert np.unique(np.abs(m[k])).size == n
    return m


def assemble(n, K, crafts, seed, window=5, kw=None, expected_sorted=0, extra=None):
    """crafts: {row: {bin: make}}.  Rows without an entry keep plain random variances."""
    rng = np.random.default_rng(seed)
    m = _matrix(rng, K, n)
    y = _plain(rng, (K, n))
    half = window // 2
    e = bin_edges(n)
    edge = np.concatenate([np.arange(half), np.arange(n - half, n)])
    for row, per_bin in sorted(crafts.items()):
        crafted = np.zeros(len(e) - 1, dtype=bool)
        crafted[list(per_bin)] = True
        if not crafted.all():  # (cases that craft every bin are built to stand a few foreign values per bin)
            # the edge loci that fell into a crafted bin exchange their x with inner loci of the other bins
            rank = np.empty(n, dtype=np.int64)
            rank[np.argsort(np.abs(m[row]))] = np.arange(n)
            bin_of = np.searchsorted(np.array(e), rank, side="right") - 1
            inner_free = np.flatnonzero(~crafted[bin_of])
            inner_free = inner_free[(inner_free >= half) & (inner_free < n - half)]
            movers = edge[crafted[bin_of[edge]]]
            partners = rng.choice(inner_free, size=movers.size, replace=False)
            m[row, movers], m[row, partners] = m[row, partners].copy(), m[row, movers].copy()
        order = np.argsort(np.abs(m[row]))
        for b, make in sorted(per_bin.items()):
            loci = order[e[b]:e[b + 1]]
            vals = make(loci.size, rng)
            assert vals.shape == (loci.size,)
            y[row, loci] = rng.permutation(vals)
    V =np.ascontiguousarray(y[:, half:n - half])
    assert V.shape == (K, n - window + 1)
    keywords = {"spatial_window": window}
    keywords.update(kw or {})
    claims = {"n": n, "K": K, "bins": len(e) - 1, "window": window, "x_distinct": True, "bin": []}
    claims.update(extra or {})
    return [np.ascontiguousarray(m), V, keywords, expected_sorted, claims]


def _claim(case, row, b, **expect):
    """Record what bin b of `row` is claimed to be, and hold the builder to it at once."""
    m, V, kw, _s, claims = case
    seen = seen_variances(V, m.shape[1], kw["spatial_window"])
    got = census(m[row], seen[row], b)
    for key, want in expect.items():
        assert got[key] == want, (key, got[key], want)
    claims["bin"].append((row, b, expect))


EVEN, ODD = 4, 10   # bins of n = 70001: widths 4118, 4117
WIDE_EVEN, WIDE_ODD, WIDE_EVEN2 = 5, 8, 10  # bins of n = 150001: widths 8334, 8333, 8334
N, N_WIDE = 70001, 150001


def _three_rows(make0, make2, claim0, claim2, seed, n=N, bins02=(EVEN, ODD), **more):
    """Row 0: the craft in an even-width bin; row 1: plain; row 2: the craft in an odd-width bin."""
    case = assemble(n, 3, {0: {bins02[0]: make0}, 2: {bins02[1]: make2}}, seed, **more)
    _claim(case, 0, bins02[0], even=True, **claim0)
    _claim(case, 2, bins02[1], even=False, **claim2)
    return case


def _cell_case(count, pos, seed, claim_more=None, **more):
    """Even bin: the upper middle value is the next of the cell, or -- the lower one being the cell's last -- the smallest value
    of the cells above, more than 2^10 times larger."""
    claim = dict(cell_count=count, cell_distinct=True, rank_in_cell=pos, padded=padded(count), count_le=(4118 - 1) // 2 + 1,
                 upper_in_cell=pos + 1 < count, upper_far=not pos + 1 < count, lower_is_cell_max=pos + 1 == count,
                 lower_is_cell_min=pos == 0)
    claim.update(claim_more or {})
    return _three_rows(craft_cell(count, pos), craft_cell(count, pos), claim, dict(claim, upper_in_cell=True, upper_far=False),
                       seed, **more)


def _run_case(length, past, same_cell_above, seed, n=N, bins02=(EVEN, ODD), **more):
    """Even bin: run_last == w/2 - 1 + past, so count_le == w/2 + past."""
    def claim(w):
        r0 = (w - 1) // 2
        return dict(run=length, run_last=r0 + past, count_le=r0 + past + 1, lower=BASE,
                    cell_count=length + same_cell_above, upper_in_cell=(past > 0 or same_cell_above > 0))
    e = bin_edges(n)
    w0, w2 = e[bins02[0] + 1] - e[bins02[0]], e[bins02[1] + 1] - e[bins02[1]]
    c0, c2 = claim(w0), claim(w2)
    c0["upper"] = BASE if past > 0 else (float(in_cell(1)) if same_cell_above else None)
    if c0["upper"] is None:
        del c0["upper"]
    return _three_rows(craft_run(length, past, same_cell_above), craft_run(length, past, same_cell_above), c0, c2, seed,
                       n=n, bins02=bins02, **more)


def _shapes_of_the_fit():
    bins = trend_bins(N)
    level = lambda rank: 1.0e-3 * 1.5 ** rank  # noqa: E731
    jitter = lambda lv: (lambda w, rng: lv * (1.0 + 0.01 * rng.random(w)))  # noqa: E731
    saw = [level(b // 2 + (6 if b % 2 else 0)) for b in range(bins)]
    crafts = {0: {b: jitter(level(b)) for b in range(bins)},
              1: {b: jitter(level(bins - 1 - b)) for b in range(bins)},
              2: {b: jitter(saw[b]) for b in range(bins)},
              3: {b: (lambda w, rng: np.full(w, 2.5e-3)) for b in range(bins)}}
    case = assemble(N, 4, crafts, 1201, kw={"min_effect": 0.25}, extra={"medians": ["increasing", "decreasing", "sawtooth", "equal"]})
    return case


def _many_segments():
    n, K = 4099, 33
    bins = trend_bins(n)
    levels = np.array([1.0e-3, 2.0e-3, 4.0e-3])
    pick = lambda w, rng: rng.choice(levels, size=w)  # noqa: E731
    crafts = {r: {b: pick for b in range(bins)} for r in range(K) if r != 17}
    return assemble(n, K, crafts, 1301, extra={"segments": 429, "levels": 3, "plain_row": 17})


def _gate(n):
    """The same craft (a run to the middle in the last bin of row 0 and in bin 5 of row 2) on both sides of the select path's
    gate and where n + 1 is a power of two in the bins expression."""
    e = bin_edges(n)
    last = len(e) - 2
    length = (e[1] - e[0]) // 4
    case = assemble(n, 3, {0: {last: craft_run(length, 0, 5)}, 2: {5: craft_run(length, 0, 5)}}, 1400 + n,
                    expected_sorted=3 if n < SELECT_MIN else 0)
    for row, b in ((0, last), (2, 5)):
        w = e[b + 1] - e[b]
        _claim(case, row, b, width=w, run=length, run_last=(w - 1) // 2, lower=BASE, cell_count=length + 5)
    return case


def _boundary_tie():
    """Row 0: two equal |x| at the ranks around the boundary of bins 6 | 7 (the sorted path: the reference's order inside the
    run, by y, decides the bins) and a run craft in bin 7, whose lowest rank is one of the two; row 1: equal |x| pairs well inside
    seven bins (the select path) and a run craft; row 2: plain."""
    case = assemble(N, 3, {0: {7: craft_run(900, 0, 40)}, 1: {EVEN: craft_run(900, 3, 40)}}, 1501, expected_sorted=1,
                    extra={"x_distinct": False})
    m, V = case[0], case[1]
    e = bin_edges(N)
    order = np.argsort(np.abs(m[0]))
    m[0, order[e[7]]] = -m[0, order[e[7] - 1]]
    order0 = order
    order = np.argsort(np.abs(m[1]))
    pairs = 0
    for b in (1, 3, EVEN, 8, 11, 14, 16):
        r = e[b] + (e[b + 1] - e[b]) // 4
        m[1, order[r + 1]] = -m[1, order[r]]
        pairs += 1
    case[4]["tie_boundary"] = (0, 7)
    case[4]["inner_pairs"] = (1, pairs)
    seen = seen_variances(V, N, 5)
    assert np.unique(np.abs(m[0])).size == N - 1 and np.unique(np.abs(m[1])).size == N - pairs
    x0 = np.sort(np.abs(m[0]))
    assert x0[e[7] - 1] == x0[e[7]]
    x1 = np.sort(np.abs(m[1]))
    assert all(x1[e[b] - 1] < x1[e[b]] for b in range(1, len(e) - 1))
    pair = order0[e[7] - 1:e[7] + 1]
    assert seen[0, pair[0]] != seen[0, pair[1]]  # (the order inside the run is decided by y)
    _claim(case, 1, EVEN, even=True, run=900, count_le=(4118 - 1) // 2 + 4, lower=BASE, upper=BASE)
    return case


def _wide_segments():
    case = assemble(N_WIDE, 2, {0: {WIDE_EVEN: craft_cell(4096, 2048), WIDE_EVEN2: craft_run(4100, 0, 50)}}, 1601)
    _claim(case, 0, WIDE_EVEN, even=True, cell_count=4096, cell_distinct=True, padded=4096, chunks=2, upper_in_cell=True)
    _claim(case, 0, WIDE_EVEN2, even=True, run=4100, run_last=8334 // 2 - 1, count_le=8334 // 2, lower=BASE,
           upper=float(in_cell(1)), cell_count=4150, chunks=2)
    case[4]["min_chunks"] = 2
    return case


BUILDERS = {
    # the largest cell that is gathered and sorted (LDS full, no padding) | the smallest that takes the counting passes
    "cell_4096": lambda: _cell_case(4096, 2048, 1001),
    "cell_4097": lambda: _cell_case(4097, 2048, 1002, kw={"prior_df": 0.0, "precision_floor_ratio": 0.5}),
    # the bitonic sort's padding: 64, 64, 128 slots
    "cell_1": lambda: _cell_case(1, 0, 1003),
    "cell_64": lambda: _cell_case(64, 10, 1004),
    "cell_65": lambda: _cell_case(65, 40, 1005, kw={"lower_bound_z": 0.0}),
    # the lower middle value at the end / at the start of its cell
    "median_last_of_cell": lambda: _cell_case(200, 199, 1006),  # (upper_far, lower_is_cell_max: claimed by _cell_case)
    "median_first_of_cell": lambda: _cell_case(200, 0, 1007),
    # runs of equal y: `long` on the counting path (n = 150001: a run of more than 4096 values cannot end at the middle of a
    # bin of 4118), `short` on the settle path
    "run_to_the_middle_long": lambda: _run_case(4100, 0, 50, 1008, n=N_WIDE, bins02=(WIDE_EVEN, WIDE_ODD)),
    "run_to_the_middle_short": lambda: _run_case(900, 0, 40, 1009),
    "run_past_the_middle_long": lambda: _run_case(4101, 100, 50, 1010, n=N_WIDE, bins02=(WIDE_EVEN, WIDE_ODD)),
    "run_past_the_middle_short": lambda: _run_case(900, 399, 40, 1011, kw={"min_effect": 0.1}),
    "floored": lambda: _three_rows(craft_floored(300), craft_floored(0),
                                   dict(lower=FLOOR, upper=FLOOR, run=(4118 - 1) // 2 + 301, run_first=0, cell_count=(4118 - 1) // 2 + 304),
                                   dict(lower=FLOOR, run=(4117 - 1) // 2 + 1, run_first=0, run_last=(4117 - 1) // 2), 1012),
    "low_bits_only": lambda: _three_rows(craft_low_bits, craft_low_bits,
                                         dict(cell_count=4118, distinct=4118, shared_high_bits=13),
                                         dict(cell_count=4117, distinct=4117, shared_high_bits=13), 1013),
    "full_range": lambda: _three_rows(craft_full_range, craft_full_range, dict(first_digits=512, distinct=4118),
                                      dict(first_digits=512, distinct=4117), 1014),
    "wide_segments": _wide_segments,
    "shapes_of_the_fit": _shapes_of_the_fit,
    "many_segments": _many_segments,
    "gate_4095": lambda: _gate(4095),
    "gate_4096": lambda: _gate(4096),
    "gate_8191": lambda: _gate(8191),
    "gate_65535": lambda: _gate(65535),
    "boundary_tie": _boundary_tie,
    "window_31": lambda: _run_case(900, 0, 40, 1015, window=31),
    "window_63": lambda: _run_case(900, 0, 40, 1016, window=63),
}
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(m, V, kwargs, expected sorted rows, claims); built once per process, read-only."""
    m, V, kw, expected_sorted, claims = BUILDERS[name]()
    m.setflags(write=False)
    V.setflags(write=False)
    return m, V, kw, expected_sorted, claims
