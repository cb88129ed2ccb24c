"""What tests/test_gpu_median_regimes.py and tests/test_median_cases_host.py share: the reference for a column median, an
independent restatement of it, and `columns(K, dtype, seed)`, a matrix of adversarial columns, one kind each, for any K.

Comparison rule (`mismatch`): values equal and NaNs in the same places, np.array_equal(got, want, equal_nan=True), so every
finite non-zero result is bit-identical.  The sign of a zero result and the sign and payload of a NaN are left free: np.median
takes them from whatever its partition happened to leave in the middle, which is no property of the column.

NumPy only: imported by a host test and by GPU tests alike."""
import numpy as np

LOW, HIGH = -3.25, 7.5  # two-valued columns: the mean of the pair (2.125) is neither of them

# every kind `columns` can emit -> (smallest K that has it, "even" where only an even K has it)
KINDS = {
    "random/distinct": (1, None), "random/ties": (1, None), "random/counts": (1, None),
    "order/ascending": (2, None), "order/descending": (2, None), "order/organ-pipe": (2, None), "order/valley": (2, None),
    "order/rotated": (2, None), "order/even-then-odd": (2, None), "order/blocks64-descending": (2, None),
    "order/blocks100-descending": (2, None),
    "inf/one-plus": (1, None), "inf/one-minus": (1, None), "inf/one-each": (2, None), "inf/plus-majority": (2, None),
    "inf/minus-majority": (2, None), "inf/plus-exactly-half": (2, "even"), "inf/half-minus-half-plus": (2, "even"),
    "inf/both-in-block64": (2, None), "inf/both-in-block100": (2, None), "inf/different-block64": (65, None),
    "inf/different-block100": (101, None),
    "nan/row-0": (1, None), "nan/row-last": (2, None), "nan/row-middle": (3, None), "nan/row-multiple-64-or-100": (65, None),
    "nan/last-real-row": (2, None), "nan/with-plus-inf": (2, None), "nan/with-minus-inf": (2, None),
    "nan/two-different-blocks": (65, None), "nan/all": (1, None),
    "mag/huge-pair-plus": (2, None), "mag/huge-pair-minus": (2, None), "mag/huge-opposite": (2, None),
    "mag/tiny-pair": (2, None), "mag/float32-subnormals": (1, None), "mag/zeros-mixed": (1, None),
    "mag/negative-zeros": (1, None), "mag/constant": (1, None),
}
for _count, _k_min in (("below-half", 4), ("half", 2), ("above-half", 3), ("above-upper-half", 4)):  # 0 < count < K
    for _place in ("random", "first", "last", "alternating"):
        KINDS[f"two/{_count}/{_place}"] = (_k_min, None)

# kinds whose columns are equal in every row on purpose
ALL_EQUAL_KINDS = ("mag/constant", "mag/negative-zeros", "mag/zeros-mixed", "nan/all")


def kinds_at(K: int):
    """The kinds a column of K rows can have (KINDS read at K)."""
    return [kind for kind, (k_min, parity) in KINDS.items() if K >= k_min and (parity is None or K % 2 == 0)]


def reference_median(m):
    """What the reference project computes (rocco/rocco.py:251, 265)."""
    with np.errstate(all="ignore"):
        return np.median(m.astype(np.float64), axis=0)


def sorted_median(m):
    """The same result from a complete sort: NaN (sorted last) in a column gives NaN, else the middle element or the mean
    of the middle pair."""
    with np.errstate(all="ignore"):
        s = np.sort(m.astype(np.float64), axis=0)
        K = s.shape[0]
        r = s[(K - 1) // 2].copy() if K % 2 else (s[K // 2 - 1] + s[K // 2]) / 2.0
        r[np.isnan(s[K - 1])] = np.nan
    return r


def mismatch(got, want, labels=None, K=None):
    """None when `got` equals `want` by the rule in the module head, else a message naming K, the kind of the first
    differing column and both values."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got, want, equal_nan=True):
        return None
    if got.shape != want.shape:
        return f"K={K}: shape {got.shape} != {want.shape}"
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    j = int(bad[0])
    kind = labels[j] if labels is not None else "?"
    return f"K={K}: {bad.size} of {got.size} columns differ; first column {j} ({kind}): got {got[j]!r}, want {want[j]!r}"


def _blocks_descending(a, L):
    return np.concatenate([a[b:b + L][::-1] for b in range(0, a.size, L)])


def _two_valued(K, count, place, rng):
    col = np.full(K, LOW)
    if place == "random":
        rows = rng.permutation(K)[:count]
    elif place == "first":
        rows = np.arange(count)
    elif place == "last":
        rows = np.arange(K - count, K)
    else:  # every other row from row 0, then the rows between them
        rows = np.concatenate([np.arange(0, K, 2), np.arange(1, K, 2)])[:count]
    col[rows] = HIGH
    return col


def _same_block_rows(K, L, rng):
    """Two rows of one block of L rows (a block that has two)."""
    blocks = [b for b in range(0, K, L) if min(L, K - b) >= 2]
    b = blocks[int(rng.integers(len(blocks)))]
    return b + rng.permutation(min(L, K - b))[:2]


def columns(K: int, dtype, seed: int):
    """(matrix [K, n] of `dtype`, labels[n]): one adversarial column per label, 130-200 of them, n no multiple of 16 (a
    partial last workgroup in every kernel).  A kind that K is too small for is left out (KINDS)."""
    dtype = np.dtype(dtype)
    f32 = dtype == np.float32
    rng = np.random.default_rng([int(seed), int(K)])
    inf, nan = np.inf, np.nan
    cols, labels = [], []

    def add(kind, col):
        k_min, parity = KINDS[kind]
        assert K >= k_min and (parity is None or K % 2 == 0), (kind, K)
        cols.append(np.asarray(col, dtype=np.float64))
        labels.append(kind)

    def finite():  # full-mantissa values
        return rng.normal(size=K)

    def distinct():  # distinct values that float32 holds exactly
        return (rng.permutation(4 * K + 8)[:K] - 2.0 * K) * 0.25

    def varied(draw):  # a short column of ties or counts is drawn again while it is constant
        col = draw()
        while K >= 2 and np.all(col == col[0]):
            col = draw()
        return col

    for _ in range(20):
        add("random/distinct", finite())
        add("random/ties", varied(lambda: np.round(rng.gamma(1.0, 0.4, size=K), 1) - 0.3))
        add("random/counts", varied(lambda: rng.poisson(0.4, size=K).astype(np.float64)))

    if K >= 2:
        a = np.sort(distinct())
        add("order/ascending", a)
        add("order/descending", a[::-1])
        add("order/organ-pipe", np.concatenate([a[0::2], a[1::2][::-1]]))
        add("order/valley", np.concatenate([a[0::2], a[1::2][::-1]])[::-1])
        add("order/rotated", np.roll(a, K // 2))
        add("order/even-then-odd", np.concatenate([a[0::2], a[1::2]]))
        add("order/blocks64-descending", _blocks_descending(a, 64))
        add("order/blocks100-descending", _blocks_descending(a, 100))

    counts = (("below-half", K // 2 - 1), ("half", K // 2), ("above-half", K // 2 + 1), ("above-upper-half", (K + 1) // 2 + 1))
    for name, count in counts:
        if 0 < count < K:
            for place in ("random", "random", "random", "first", "last", "alternating"):
                add(f"two/{name}/{place}", _two_valued(K, count, place, rng))

    for _ in range(2):
        for kind, value in (("inf/one-plus", inf), ("inf/one-minus", -inf)):
            col = finite()
            col[rng.integers(K)] = value
            add(kind, col)
        if K < 2:
            continue
        order = rng.permutation(K)
        col = finite()
        col[order[0]], col[order[1]] = inf, -inf
        add("inf/one-each", col)
        for kind, value in (("inf/plus-majority", inf), ("inf/minus-majority", -inf)):
            col = finite()
            col[rng.permutation(K)[:K // 2 + 1]] = value
            add(kind, col)
        if K % 2 == 0:
            col = finite()
            col[rng.permutation(K)[:K // 2]] = inf
            add("inf/plus-exactly-half", col)
            col = np.full(K, inf)
            col[rng.permutation(K)[:K // 2]] = -inf
            add("inf/half-minus-half-plus", col)
        for L in (64, 100):
            col = finite()
            r = _same_block_rows(K, L, rng)
            col[r[0]], col[r[1]] = inf, -inf
            add(f"inf/both-in-block{L}", col)
            if K > L:
                col = finite()
                first = inf if rng.random() < 0.5 else -inf
                col[rng.integers(0, L)], col[rng.integers(L, K)] = first, -first
                add(f"inf/different-block{L}", col)

    nan_rows = [("nan/row-0", 0)]
    if K >= 2:
        nan_rows.append(("nan/row-last", K - 1))
    if K >= 3:
        nan_rows.append(("nan/row-middle", K // 2))
    nan_rows += [("nan/row-multiple-64-or-100", r) for r in sorted(set(range(64, K, 64)) | set(range(100, K, 100)))]
    for kind, r in nan_rows:
        col = finite()
        col[r] = nan
        add(kind, col)
    if K >= 2:
        col = np.sort(distinct())  # the NaN sits where the largest value would: the last real row before the padding
        col[K - 1] = nan
        add("nan/last-real-row", col)
        for kind, value in (("nan/with-plus-inf", inf), ("nan/with-minus-inf", -inf)):
            col = finite()
            order = rng.permutation(K)
            col[order[0]], col[order[1]] = nan, value
            add(kind, col)
    if K > 64:
        col = finite()
        col[rng.integers(0, 64)] = nan
        col[rng.integers(max(64, min(100, K - 1)), K)] = nan
        add("nan/two-different-blocks", col)
    add("nan/all", np.full(K, nan))

    # float32 holds neither 1.7e308 nor 5e-324: its own largest value and smallest subnormals stand in for them
    huge = float(np.finfo(np.float32).max) if f32 else 1.7e308
    tiny = (2.0 ** -149, 2.0 ** -148) if f32 else (5e-324, 1e-323)
    if K >= 2:
        col = finite()
        col[rng.permutation(K)[:min(K, (K + 1) // 2 + 1)]] = huge  # the middle pair is (huge, huge)
        add("mag/huge-pair-plus", col)
        add("mag/huge-pair-minus", -col)
        col = np.full(K, huge)
        col[rng.permutation(K)[:K // 2]] = -huge
        add("mag/huge-opposite", col)
        below = (K - 1) // 2
        col = np.concatenate([-1.0 - np.abs(rng.normal(size=below)), tiny, 1.0 + np.abs(rng.normal(size=K - below - 2))])
        add("mag/tiny-pair", rng.permutation(col))
    add("mag/float32-subnormals", rng.integers(1, 2 ** 23, size=K) * 2.0 ** -149 * rng.choice([-1.0, 1.0], size=K))
    add("mag/zeros-mixed", np.where(rng.random(K) < 0.5, -0.0, 0.0))
    add("mag/negative-zeros", np.full(K, -0.0))
    add("mag/constant", np.full(K, np.round(rng.normal(), 3)))

    while len(cols) % 16 == 0 or len(cols) < 130:
        add("random/distinct", finite())
    with np.errstate(all="ignore"):
        matrix = np.ascontiguousarray(np.stack(cols, axis=1).astype(dtype))
    assert matrix.shape == (K, len(labels)) and len(labels) % 16 != 0
    return matrix, labels


def two_valued_exhaustive(K: int):
    """[K, 2**K] float64: every assignment of LOW / HIGH to the K rows (column c has HIGH in row k where bit k of c is set)."""
    bits = (np.arange(2 ** K, dtype=np.int64)[None, :] >> np.arange(K, dtype=np.int64)[:, None]) & 1
    return np.where(bits == 1, HIGH, LOW)


def two_valued_balanced(K: int, n: int, seed: int):
    """[K, n] float64: columns of LOW / HIGH at random rows, the number of HIGH within two of K // 2 -- the columns on which a
    selection of the middle pair can go wrong at all."""
    rng = np.random.default_rng([int(seed), int(K), int(n)])
    count = np.clip(K // 2 + rng.integers(-2, 3, size=n), 0, K)
    m = np.where(np.arange(K)[:, None] < count[None, :], HIGH, LOW)
    return np.ascontiguousarray(rng.permuted(m, axis=0))


_SWEEP = {"1-100": (1, 100), "101-200": (101, 200), "201-256": (201, 256), "257-300": (257, 300), "301-600": (301, 600),
          "601-900": (601, 900), "901-1210": (901, 1210)}  # (the issue's 601-1210 in two: each stays within seconds)
_NETWORKS = (20, 24, 32, 40, 50, 64, 80, 100)
_REGIMES = {
    "host": [1, 2, 3, 16, 17, 100, 101, 199, 256, 300, 301, 1200, 1201],
    "exhaustive": list(range(2, 21)),  # 2**K columns: a proof for KP = 2 ... 16, and for 20 exact and padded
    "sampled-24": [21, 22, 23, 24],
    "balanced-networks": sorted(k - d for k in _NETWORKS for d in (0, 1, 3)),
    "balanced-large": [101, 150, 199, 200, 201, 255, 256, 257, 299, 300, 301, 450, 599, 600, 601, 900, 1199, 1200],
    "batch": list(range(2, 101)),
    "batch-fallback": [101, 150],
    "methods": [2, 3, 7, 8, 9, 15, 16, 17, 100, 127, 128, 129, 130, 143, 144, 257, 264, 1024, 1025],
}
_REGIMES.update({f"sweep-{name}": list(range(lo, hi + 1)) for name, (lo, hi) in _SWEEP.items()})
SWEEP_RANGES = tuple(_SWEEP)


def ks_for(regime: str):
    """The K list of a regime of tests/test_gpu_median_regimes.py ("sweep-<range>" for the ranges of SWEEP_RANGES)."""
    return list(_REGIMES[regime])
