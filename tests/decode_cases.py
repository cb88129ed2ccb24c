"""What tests/test_decode_cases_host.py and tests/test_gpu_decode_edges.py share: named solution vectors for the kernels of
rocco_amd/csrc/decode.hip, the runs they must decode to, and a census of what each vector makes the kernels do.

The kernels' geometry, restated here so that the host test can say which paths a case reaches: a lane reads LANE = 16
loci, a wavefront 64 lanes = WAVE loci, a workgroup of 256 lanes one TILE = 4096 loci; the scan kernels are one workgroup
of 1024 lanes with one tile per lane, so one scan TRIP covers 1024 tiles = 4 194 304 loci and longer vectors pass a carry
from trip to trip.  decode_table_to_host_kernel runs 256 x 256 lanes that move two table words each per grid stride.

Expected runs are an independent statement of rocco/rocco.py:180-190: loci 0..n-2 with a non-zero byte are selected, the
last locus never, touching loci merge (`expected_runs`).

NumPy only, deterministic (fixed seeds), no device."""
import numpy as np

LANE = 16
WAVE = 64 * LANE
TILE = 256 * LANE
TRIP = 1024 * TILE
BOUNDARIES = {"lane": LANE, "wave": WAVE, "tile": TILE, "trip": TRIP}
HOST_COPY_LANES = 256 * 256       # lanes of decode_table_to_host_kernel, 2 words (16 bytes) each per stride
BATCH_MAX = 48                    # tasks of one batch or table call (kDecodeBatchMax)

N_ONE_TRIP = TRIP                 # exactly one scan trip
N_TWO_TRIPS = TRIP + 1            # a second trip that holds one tile
N_THREE_TRIPS = 2 * TRIP + TILE + 1
LARGE_SIZES = (N_ONE_TRIP, N_TWO_TRIPS, N_THREE_TRIPS)
EDGE_SIZES = tuple([2, 3] + [b * k + d for b in (LANE, TILE) for k in (1, 2) for d in (-2, -1, 0, 1, 2)])
DENSE_N = 400001                  # 1010...: 200 000 runs
MID_N = 120001                    # 1010...: 60 000 runs, the second stride of the to-host kernel and no third
PLACED_SIZES = (TILE + 2, 2 * TILE + 1)   # 4098: locus 4096 is n-2;  8193: two tiles and one locus
PLACED_LOCI = (0, 15, 16, 1023, 1024, 4095, 4096)
BYTE_VALUES = (2, 0x80, 0xFF)


def expected_runs(z):
    """(begins, ends) of the maximal runs of non-zero bytes among loci 0..n-2, ends exclusive, as int64 arrays."""
    z = np.asarray(z)
    d = np.diff(np.concatenate([[0], (z[:-1] != 0).astype(np.int8), [0]]))
    return np.flatnonzero(d == 1).astype(np.int64), np.flatnonzero(d == -1).astype(np.int64)


def scan_trips(n):
    tiles = -(-n // TILE)
    return -(-tiles // 1024)


def host_copy_strides(rows):
    """Grid strides decode_table_to_host_kernel takes for a table of `rows` rows."""
    pairs = (3 * rows + 1) // 2
    return -(-pairs // HOST_COPY_LANES)


# ------------------------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------------------------
def _zeros(n):
    return np.zeros(n, dtype=np.uint8)


def _ones(n):
    return np.ones(n, dtype=np.uint8)


def _alt(n, first):
    z = np.zeros(n, dtype=np.uint8)
    z[(0 if first else 1)::2] = 1
    return z


def _rand(n, seed, p=0.3):
    return (np.random.default_rng(seed).random(n) < p).astype(np.uint8)


def _loci(n, loci):
    z = np.zeros(n, dtype=np.uint8)
    z[list(loci)] = 1
    return z


def _sparse(n, seed, placed, patches):
    """About one short run per 1000 loci, `placed` runs [lo, hi) and 64-locus 1010 patches starting at `patches`."""
    rng = np.random.default_rng(seed)
    z = np.zeros(n, dtype=np.uint8)
    starts = rng.integers(0, n, size=n // 1000)
    lengths = rng.integers(1, 30, size=starts.size)
    for s, k in zip(starts.tolist(), lengths.tolist()):
        z[s:s + k] = 1
    for lo in patches:
        z[lo:lo + 64] = 0
        z[lo:lo + 64:2] = 1
    for lo, hi in placed:
        z[max(lo - 2, 0):hi + 2] = 0  # (clear of the random runs, so that the run is exactly [lo, hi))
        z[lo:hi] = 1
    return z


def _revalue(builder, value, seed=0):
    """The same vector with every selected byte replaced by `value` (None: a seeded mix of non-zero bytes)."""
    def build():
        z = builder().copy()
        if value is None:
            mix = np.random.default_rng(seed).choice(np.array([1, 2, 3, 0x7F, 0x80, 0xFE, 0xFF], dtype=np.uint8), size=z.size)
            return np.where(z != 0, mix, 0).astype(np.uint8)
        z[z != 0] = value
        return z
    return build


def _bind(fn, *args, **kwargs):
    return lambda: fn(*args, **kwargs)


BYTE_VALUE_ORIGINALS = ("rand@4097", "alt10@33", "run[n-3,n)@8193")


def cases():
    """[(name, n, builder)]; builder() -> uint8 vector of length n."""
    out = [(f"alt10@{MID_N}", MID_N, _bind(_alt, MID_N, True))]  # (first: a call of its own kind, away from the 200 000-row cases)
    for n in EDGE_SIZES:
        out.append((f"zeros@{n}", n, _bind(_zeros, n)))
        out.append((f"ones@{n}", n, _bind(_ones, n)))
        out.append((f"alt10@{n}", n, _bind(_alt, n, True)))
        out.append((f"alt01@{n}", n, _bind(_alt, n, False)))
        out.append((f"rand@{n}", n, _bind(_rand, n, 7000 + n)))
    out.append((f"alt10@{DENSE_N}", DENSE_N, _bind(_alt, DENSE_N, True)))
    out.append((f"alt01@{DENSE_N}", DENSE_N, _bind(_alt, DENSE_N, False)))
    for n in PLACED_SIZES:
        singles = sorted(set(p for p in PLACED_LOCI + (n - 2, n - 1) if p < n))
        for p in singles:
            out.append((f"single[{p}]@{n}", n, _bind(_loci, n, (p,))))
        for p in sorted(set(q for q in (0, 15, 1023, 4095, n - 2) if q + 1 < n)):
            out.append((f"pair[{p},{p + 1}]@{n}", n, _bind(_loci, n, (p, p + 1))))
    for n in (3, 18) + PLACED_SIZES:
        name = f"run[n-3,n)@{n}"
        if name not in [c[0] for c in out]:
            out.append((name, n, _bind(_loci, n, (n - 3, n - 2, n - 1))))
    # the multi-trip sizes: one run through everything, and sparse runs with the trip boundaries placed on purpose
    for n in LARGE_SIZES:
        out.append((f"ones@{n}", n, _bind(_ones, n)))
    n = N_ONE_TRIP
    out.append((f"sparse@{n}", n, _bind(_sparse, n, 11, [(n - 3, n), (TILE * 1023 - 1, TILE * 1023 + 1)], [TILE * 512 - 32, n - 200])))
    n = N_TWO_TRIPS
    out.append((f"sparse@{n}", n, _bind(_sparse, n, 12, [(TRIP - 5, n)], [TILE * 1023 - 32, 5000])))  # clipped: ends AT the trip boundary
    n = N_THREE_TRIPS
    out.append((f"sparse-cross@{n}", n,
                _bind(_sparse, n, 13, [(TRIP - 1, TRIP + 1), (2 * TRIP - 7, 2 * TRIP + 9), (n - 3, n)], [TRIP + 100, 2 * TRIP + TILE - 40])))
    out.append((f"sparse-touch@{n}", n,
                _bind(_sparse, n, 14, [(TRIP - 14, TRIP), (2 * TRIP, 2 * TRIP + 3), (2 * TRIP + TILE - 1, 2 * TRIP + TILE)],
                      [TRIP - 200, 2 * TRIP - 64])))
    # bytes other than 0 and 1
    by_name = {name: (n, b) for name, n, b in out}
    for orig in BYTE_VALUE_ORIGINALS:
        n, b = by_name[orig]
        for v in BYTE_VALUES:
            out.append((f"{orig}#0x{v:02X}", n, _revalue(b, v)))
    n, b = by_name["rand@8194"]
    out.append(("rand@8194#mix", n, _revalue(b, None, seed=99)))
    return out


def original_of(name):
    """The case a byte-value variant was made from, or None."""
    return name.split("#")[0] if "#" in name else None


# ------------------------------------------------------------------------------------------------------------------
# census
# ------------------------------------------------------------------------------------------------------------------
def census(z, begins=None, ends=None):
    """What vector `z` makes the decode kernels do: scan trips, rows, row parity, the most run starts in one 16-locus lane,
    and per boundary kind which of 'start' (a run begins on a multiple, other than 0), 'end' (a run's exclusive end is a
    multiple) and 'cross' (a run holds the loci on both sides of a multiple) occur."""
    n = int(z.shape[0])
    if begins is None:
        begins, ends = expected_runs(z)
    rows = int(begins.size)
    touched = {}
    for kind, b in BOUNDARIES.items():
        how = set()
        if rows:
            if np.any((begins % b == 0) & (begins > 0)):
                how.add("start")
            if np.any(ends % b == 0):
                how.add("end")
            if np.any(begins // b < (ends - 1) // b):
                how.add("cross")
        touched[kind] = how
    return {
        "n": n,
        "trips": scan_trips(n),
        "rows": rows,
        "odd_rows": bool(rows & 1),
        "max_starts_in_lane": int(np.bincount(begins // LANE).max()) if rows else 0,
        "boundaries": touched,
        "nonzero": bool(np.any(z != 0)),
    }


# ------------------------------------------------------------------------------------------------------------------
# packing into batch / table calls
# ------------------------------------------------------------------------------------------------------------------
def batches(case_list=None):
    """The case list cut into calls of at most BATCH_MAX cases, in list order, except that every multi-trip case is moved
    behind the first small case of its call (its first tile is then not tile 0 of the launch)."""
    case_list = cases() if case_list is None else case_list
    out = []
    for at in range(0, len(case_list), BATCH_MAX):
        part = list(case_list[at:at + BATCH_MAX])
        small = [c for c in part if scan_trips(c[1]) == 1 and c[1] < TRIP]
        large = [c for c in part if c not in small]
        if large:
            if not small:
                raise ValueError("a call of multi-trip cases only")
            part = small[:1] + large + small[1:]
        out.append(part)
    return out
