"""What tests/test_gpu_baseline_seams.py and tests/test_baseline_cases_host.py share: the matrices that take the batched
baseline sweeps (rocco_amd/csrc/whittaker.hip) to the edges of their segment plan, a plain sequential restatement of one
row's cross-fit Whittaker baseline, and `seam_meets`, which says whether a segment's warm-up reaches the row's own bits.

The restatement follows the project's statement of the algorithm (whittaker.hip): the factor
recurrence, rhs = W_p y, the forward substitution, z = f / d, the backward substitution, 0.5 (x0 + x1) -- Python floats,
every product and difference rounded on its own, no fused multiply-add.  It is pinned against the oracle bit for bit by
the host test.

A case's `label` says what its seams do at its forced settings: "forced" -- at least one seam's warm-up does not reach the
true state's bits (the seam kernel must recompute, the repair counter rises); "met" -- every seam meets (the counter
stays); None -- no claim.  The host test certifies every label with `seam_meets`; the GPU test asserts the counter by it.

NumPy only: imported by a host test and by GPU tests alike."""
import functools

import numpy as np

TILE = 64
WINDOWS = (3, 9, 101, 1001)


def penalty(window: int) -> float:
    """The Whittaker penalty of a smoothing window, through the package's own rule."""
    from rocco_amd.inference import _consenrich_whittaker_lambda

    return _consenrich_whittaker_lambda(window)


# ---- one row, sequentially ------------------------------------------------------------------------------------------------

def _a0(i, n, parity, lam):
    w = 1.0 if (i & 1) == parity else 0.0
    if i == 0 or i == n - 1:
        return w + lam
    if i == 1 or i == n - 2:
        return w + (5.0 * lam)
    return w + (6.0 * lam)


def _a1(i, n, lam):
    return (-2.0 * lam) if (i == 0 or i == n - 2) else (-4.0 * lam)


@functools.lru_cache(maxsize=64)
def factor(n: int, lam: float, parity: int):
    """d[n], l1[n - 1], l2[n - 2] of W_p + lam D^T D = L D L^T (lists; l1 / l2 padded with 0.0 to n entries)."""
    assert n >= 25
    d, l1, l2 = [0.0] * n, [0.0] * n, [0.0] * n
    d[0] = _a0(0, n, parity, lam)
    l1[0] = _a1(0, n, lam) / d[0]
    l2[0] = lam / d[0]
    d[1] = _a0(1, n, parity, lam) - ((l1[0] * l1[0]) * d[0])
    l1[1] = (_a1(1, n, lam) - ((l2[0] * d[0]) * l1[0])) / d[1]
    l2[1] = lam / d[1]
    for i in range(2, n):
        t1 = (l1[i - 1] * l1[i - 1]) * d[i - 1]
        t2 = (l2[i - 2] * l2[i - 2]) * d[i - 2]
        d[i] = _a0(i, n, parity, lam) - t1 - t2
        if i + 2 <= n:
            t1 = (l2[i - 1] * d[i - 1]) * l1[i - 1]
            l1[i] = (_a1(i, n, lam) - t1) / d[i]
        if i + 3 <= n:
            l2[i] = lam / d[i]
    return d, l1, l2


def rhs_value(y: float, i: int, n: int, parity: int) -> float:
    """W_p y at locus i: the two entries at either end are selected, the others multiplied by the 0 / 1 weight (the
    product decides the sign of a zero, and 0 x inf is NaN)."""
    mine = (i & 1) == parity
    if i < 2 or i + 2 >= n:
        return y if mine else 0.0
    return (1.0 if mine else 0.0) * y


class RowSolve:
    """One row's sequential solve: per parity p the forward substitution f[p] (before its division), z[p] = f / d, the
    backward substitution x[p]; baseline = 0.5 (x[0] + x[1])."""

    def __init__(self, row, lam: float):
        y = [float(v) for v in np.asarray(row, dtype=np.float64)]
        n = len(y)
        self.n, self.lam, self.y = n, float(lam), y
        self.v, self.f, self.z, self.x = [None, None], [None, None], [None, None], [None, None]
        for p in (0, 1):
            d, l1, l2 = factor(n, self.lam, p)
            v = [rhs_value(y[i], i, n, p) for i in range(n)]
            f = list(v)
            f[1] = f[1] - (l1[0] * f[0])
            for i in range(2, n):
                t1 = l1[i - 1] * f[i - 1]
                t2 = l2[i - 2] * f[i - 2]
                f[i] = f[i] - t1 - t2
            with np.errstate(all="ignore"):
                z = (np.array(f) / np.array(d)).tolist()
            x = [0.0] * n
            x[n - 1] = z[n - 1]
            x[n - 2] = z[n - 2] - (l1[n - 2] * x[n - 1])
            for i in range(n - 3, -1, -1):
                t1 = l1[i] * x[i + 1]
                t2 = l2[i] * x[i + 2]
                x[i] = z[i] - t1 - t2
            self.v[p], self.f[p], self.z[p], self.x[p] = v, f, z, x
        with np.errstate(all="ignore"):
            self.baseline = 0.5 * (np.array(self.x[0]) + np.array(self.x[1]))

    def chain_state(self, parity: int, sweep: str, locus: int):
        """(value at `locus`, the value one step earlier in sweep order) of the forward chain f or the backward chain x; a
        step that lies outside the row is the chains' zero start."""
        if sweep == "forward":
            seq, earlier = self.f[parity], locus - 1
        else:
            seq, earlier = self.x[parity], locus + 1
        return seq[locus], (seq[earlier] if 0 <= earlier < self.n else 0.0)


def baseline_row(row, lam: float) -> np.ndarray:
    return RowSolve(row, lam).baseline


def baseline_matrix(matrix, lam: float) -> np.ndarray:
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape[1] < 25:
        return np.zeros_like(m)
    return np.stack([baseline_row(r, lam) for r in m])


def _bits(x: float) -> bytes:
    return np.float64(x).tobytes()


def _chain_step(v, c1, c2, p1, p2):
    t1 = c1 * p1
    t2 = c2 * p2
    return v - t1 - t2


def seam_meets(row, lam: float, parity: int, sweep: str, seam_locus: int, warm_loci: int) -> bool:
    """Does a segment's warm-up reach the row's own bits at a seam?  `seam_locus`: the first locus above the seam (a
    multiple of the tile).  Forward: the chain started from the zero state at max(0, seam_locus - warm_loci) against the
    true state (f[seam_locus - 1], f[seam_locus - 2]); backward: the chain started from the zero state at
    min(n, seam_locus + warm_loci) - 1, walking down, against (x[seam_locus], x[seam_locus + 1]).  A warm-up clipped at
    the row's end IS the row's own sweep.  `row`: the values the sweeps read (matrix - offset of the row), or a RowSolve."""
    s = row if isinstance(row, RowSolve) else RowSolve(row, lam)
    n = s.n
    assert 0 < seam_locus < n and seam_locus % TILE == 0 and warm_loci > 0 and warm_loci % TILE == 0
    _d, l1, l2 = factor(n, s.lam, parity)
    p1 = p2 = 0.0
    if sweep == "forward":
        v = s.v[parity]
        for i in range(max(0, seam_locus - warm_loci), seam_locus):
            a = l1[i - 1] if i >= 1 else 0.0
            b = l2[i - 2] if i >= 2 else 0.0
            p1, p2 = _chain_step(v[i], a, b, p1, p2), p1
        t1, t2 = s.chain_state(parity, "forward", seam_locus - 1)
    else:
        z = s.z[parity]
        for i in range(min(n, seam_locus + warm_loci) - 1, seam_locus - 1, -1):
            a = l1[i] if i < n - 1 else 0.0
            b = l2[i] if i < n - 2 else 0.0
            p1, p2 = _chain_step(z[i], a, b, p1, p2), p1
        t1, t2 = s.chain_state(parity, "backward", seam_locus)
    return _bits(p1) == _bits(t1) and _bits(p2) == _bits(t2)


# ---- the plan at forced settings ---------------------------------------------------------------------------------------------

def forced_plan(cols: int, segment: int, warm: int):
    """(n_seg, seg_tiles, warm_tiles) of a row of `cols` loci under ROCCO_HIP_WHITTAKER_SEGMENT_LOCI = segment and
    _WARM_LOCI = warm, restated from whittaker.hip's comments: about cols / segment pieces of whole tiles, none for a row
    shorter than two segments.  The GPU tests assert that the library's plan query says the same."""
    tiles = -(-cols // TILE)
    pieces = (cols + segment // 2) // segment if (segment > 0 and cols >= 2 * segment) else 1
    n_seg, seg_tiles = 1, tiles
    if pieces > 1 and cols >= 25:
        seg_tiles = -(-tiles // pieces)
        n_seg = -(-tiles // seg_tiles)
    if n_seg < 2:
        n_seg, seg_tiles = 1, tiles
    return n_seg, seg_tiles, -(-max(TILE, warm) // TILE)


def seams_of(cols: int, segment: int, warm: int):
    """The loci at which a row is cut."""
    n_seg, seg_tiles, _w = forced_plan(cols, segment, warm)
    return [s * seg_tiles * TILE for s in range(1, n_seg)]


def every_warm_up_is_the_rows_own_sweep(cols: int, segment: int, warm: int) -> bool:
    """True when every segment's warm-up reaches back to the row's start and on to its end: then every seam meets whatever
    the data."""
    n_seg, seg_tiles, warm_tiles = forced_plan(cols, segment, warm)
    tiles = -(-cols // TILE)
    return (n_seg - 1) * seg_tiles <= warm_tiles and seg_tiles + warm_tiles >= tiles


def first_length(holds, start: int, stop: int) -> int:
    """A length c in (start, stop] with holds(c) and not holds(c - 1), the first one a tile-by-tile walk up from `start`
    comes to.  `holds` asks the library's plan query (default settings: the plan depends on the resident workgroups, so
    the GPU tests take their lengths from it and not from a constant)."""
    assert not holds(start)
    c = start + TILE
    while c <= stop and not holds(c):
        c += TILE
    assert c <= stop, "no such length"
    while holds(c - 1):
        c -= 1
    return c


class Case:
    def __init__(self, name, label, segment, warm, lam, matrix, offsets=None):
        self.name, self.label, self.segment, self.warm, self.lam = name, label, int(segment), int(warm), float(lam)
        self.matrix = np.ascontiguousarray(matrix, dtype=np.float64)
        self.offsets = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.float64)
        self.rows, self.cols = self.matrix.shape

    def plan(self):
        return forced_plan(self.cols, self.segment, self.warm)

    def seams(self):
        return seams_of(self.cols, self.segment, self.warm)

    def sweep_input(self, form: str):
        """What the sweeps read: the matrix (baseline form), the matrix minus the rows' offsets (residual form)."""
        if form == "baseline" or self.offsets is None:
            return self.matrix
        return self.matrix - self.offsets[:, None]

    def __repr__(self):
        return f"Case({self.name}: {self.rows} x {self.cols}, segment {self.segment}, warm {self.warm}, {self.label})"


def open_seams(case: Case, form: str = "baseline", rows=None, first_only: bool = False):
    """[(row, sweep, parity, seam locus)] of the seams that do not meet, by seam_meets."""
    found = []
    g = case.sweep_input(form)
    for r in (range(case.rows) if rows is None else rows):
        solve = RowSolve(g[r], case.lam)
        for sweep in ("forward", "backward"):
            for parity in (0, 1):
                for seam in case.seams():
                    if not seam_meets(solve, case.lam, parity, sweep, seam, -(-case.warm // TILE) * TILE):
                        found.append((r, sweep, parity, seam))
                        if first_only:
                            return found
    return found


def _seed(*parts) -> int:
    return int(sum((i + 1) * 7919 * int(p) for i, p in enumerate(parts)) % (2 ** 31))


def _gauss(rows, cols, *seed, scale=2.0, centre=0.0):
    return np.random.default_rng(_seed(*seed)).normal(centre, scale, size=(rows, cols))


# ---- D1: segments of 1 to 4 tiles ------------------------------------------------------------------------------------------

D1_SEGMENTS, D1_WARMS, D1_ROWS = (64, 128, 192), (64, 128, 256), (1, 17)


def d1_cols(segment: int):
    return (2 * segment, 2 * segment + 1, 3 * segment + 63, 4 * segment + 64, 5 * segment - 1)


def d1_cases(segment: int, warm: int):
    """Window 101; Gaussian rows about 3 with their medians as offsets.  "met" only where every warm-up is the row's own
    sweep (a warm-up of 64 to 256 loci reaches nothing at this penalty)."""
    lam = penalty(101)
    for cols in d1_cols(segment):
        for rows in D1_ROWS:
            m = _gauss(rows, cols, 1, segment, warm, cols, rows, centre=3.0)
            label = "met" if every_warm_up_is_the_rows_own_sweep(cols, segment, warm) else "forced"
            yield Case(f"d1/S{segment}/W{warm}/{rows}x{cols}", label, segment, warm, lam, m, np.median(m, axis=1))


# ---- D2: the seam kernel past its first wavefront ---------------------------------------------------------------------------

D2_ROWS, D2_SEGMENT, D2_WARM, D2_COLS = (63, 64, 65, 129), 1024, 64, 4097


def d2_case(rows: int):
    m = _gauss(rows, D2_COLS, 2, rows)
    return Case(f"d2/{rows}x{D2_COLS}", "forced", D2_SEGMENT, D2_WARM, penalty(101), m, np.median(m, axis=1))


# (rows, cols, segments per row) of the batch, in its order: cut, uncut, too short for a baseline, cut otherwise, two groups
D2_BATCH = ((65, 4097, 4), (3, 1500, 1), (4, 24, 0), (2, 2100, 2), (17, 3000, 3))


def d2_batch():
    out = []
    for k, (rows, cols, n_seg) in enumerate(D2_BATCH):
        m = _gauss(rows, cols, 3, k)
        out.append(Case(f"d2/batch{k}/{rows}x{cols}", "forced" if n_seg > 1 else None, D2_SEGMENT, D2_WARM, penalty(101), m,
                        np.median(m, axis=1)))
    return out


# ---- D3: penalties ----------------------------------------------------------------------------------------------------------

D3_SEGMENT = D3_WARM = 4096
D3_SHAPE = (5, 6 * 4096 + 17)
# what 4096 loci of warm-up do at each window's penalty, certified by the host test
D3_LABELS = {3: "met", 9: "met", 101: "forced", 1001: "forced"}


def d3_case(window: int):
    return Case(f"d3/window{window}", D3_LABELS[window], D3_SEGMENT, D3_WARM, penalty(window), _gauss(*D3_SHAPE, 4, window))


# ---- D4: adversarial rows ---------------------------------------------------------------------------------------------------

D4_SEGMENT, D4_WARM, D4_ROWS, D4_COLS = 2048, 512, 8, 6 * 2048 + 17
D4_KINDS = ("spike-1e6", "spike-1e290", "step-at-seam", "constant-beside-zero", "zeros-and-denormals", "blocks-1e-290-1e200")
# (certified by the host test; the rows of zeros of either sign meet, the all-zero rows too: one open seam makes "forced")
D4_LABELS = {"spike-1e6": "forced", "spike-1e290": "forced", "step-at-seam": "forced", "constant-beside-zero": "forced",
             "zeros-and-denormals": "forced", "blocks-1e-290-1e200": "forced", "inf-in-row-3": "forced"}
D4_INF_ROW = 3


def d4_case(kind: str):
    rows, cols = D4_ROWS, D4_COLS
    seams = seams_of(cols, D4_SEGMENT, D4_WARM)
    rng = np.random.default_rng(_seed(5, D4_KINDS.index(kind) if kind in D4_KINDS else 99))
    m = np.zeros((rows, cols))
    if kind in ("spike-1e6", "spike-1e290"):
        # rows 0-3: noise up to the spike; rows 4-7: nothing but the spike; exact zeros from the spike to the row's end
        for r in range(rows):
            at = seams[r % len(seams)] - 1 - 3 * (r // len(seams))
            if r < 4:
                m[r, :at] = rng.normal(0.0, 2.0, size=at)
            m[r, at] = 1e6 if kind == "spike-1e6" else 1e290
    elif kind == "step-at-seam":
        for r in range(rows):
            m[r, seams[r % len(seams)]:] = 50.0
            if r >= 5:
                m[r] += rng.normal(0.0, 0.5, size=cols)
    elif kind == "constant-beside-zero":
        for r, c in zip(range(0, rows, 2), (3.75, -2.5, 1e5, 1.0 / 3.0)):
            m[r] = c
    elif kind == "zeros-and-denormals":
        m[1] = -0.0
        m[2, ::2] = -0.0
        m[3] = 1e-310
        m[4] = np.where(rng.integers(0, 2, size=cols) == 1, 1e-310, -1e-310)
        m[5] = np.where(rng.integers(0, 3, size=cols) == 0, 1e-310, -0.0)
        m[6] = 5e-324
        m[7, seams[2] - 1] = -0.0
        m[7, seams[3]] = 1e-310
    elif kind == "blocks-1e-290-1e200":
        for r, block in enumerate((1, 7, 64, 100, 513, 2048, 2112, 33)):
            which = (np.arange(cols) // block) & 1
            m[r] = np.where(which == 1, 1e200, 1e-290)
            if r % 2 == 1:
                m[r] *= np.where(rng.integers(0, 2, size=cols) == 1, 1.0, -1.0)
    elif kind == "inf-in-row-3":
        m = rng.normal(0.0, 2.0, size=(rows, cols))
        m[D4_INF_ROW, seams[1] + 5] = np.inf
    else:
        raise KeyError(kind)
    return Case(f"d4/{kind}", D4_LABELS[kind], D4_SEGMENT, D4_WARM, penalty(101), m)


# ---- D5: a cut row under a longer factor ------------------------------------------------------------------------------------

D5_SEGMENT, D5_WARM, D5_LONG = 1024, 64, (3, 40001)
D5_SHAPES = ((5, 8200), (4, 8193))
D5_PENALTIES = (12345.678, 23456.789)  # (no other test uses them: the device's factor of each is built by this test)


def d5_long(lam: float):
    return _gauss(*D5_LONG, 6, int(lam))


def d5_cases(lam: float):
    return [Case(f"d5/{rows}x{cols}", "forced", D5_SEGMENT, D5_WARM, lam, _gauss(rows, cols, 7, int(lam), cols)) for rows, cols in D5_SHAPES]
