"""What tests/test_gpu_launch_turns.py and tests/test_launch_turns_sizes.py share: the sizes at which the record and select
kernels enter their second turn, computed from the caps the library states (rocco_hip_launch_caps, include/rocco_hip.h),
and the inputs built at those sizes.

Every kernel concerned caps its grid; past cap x unit a workgroup takes several units in turn.  A size here is
cap x unit + a few units + an odd remainder: some workgroups take two units, the others one.  Every builder puts the fact
that decides the answer where only a later turn reads it (or, for a mirror case, only the first), so a kernel that reads
one turn, or one turn twice, gives another answer.  Each `*_sizes` function asserts that premise from the caps alone: a
changed cap that would turn a case back into a first-turn case fails there, without a GPU."""
import functools
import struct

import numpy as np

import bam_expected as bx


def caps():
    from rocco_amd import _native

    return _native.launch_caps()


def second_turn(items: int, unit: int, cap: int) -> int:
    """The first item of the second turn of a launch of min(ceil(items / unit), cap) workgroups that take `unit` items per
    turn; asserts that some workgroups take two units and the others one."""
    units = -(-items // unit)
    assert cap < units < 2 * cap, f"{items} items in units of {unit} under a cap of {cap}: no workgroup takes a second unit, or every one does"
    assert items % unit != 0, "the last unit is a whole one"
    return cap * unit


# ---- the select --------------------------------------------------------------------------------------------------------
def select_blocks(lengths, c):
    """(blocks, chunks) per vector of one group: the dealing rule of include/rocco_hip.h."""
    total = sum(int(n) for n in lengths)
    out = []
    for n in lengths:
        chunks = -(-int(n) // c["select_chunk_values"])
        share = int(float(c["select_grid_target"]) * float(n) / float(max(total, 1))) + 1
        out.append((min(chunks, share), chunks))
    return out


def select_single_size(c) -> int:
    n = c["select_grid_target"] * c["select_chunk_values"] + 5 * c["select_chunk_values"] + 77
    ((blocks, chunks),) = select_blocks([n], c)
    assert blocks < chunks < 2 * blocks and n < 2 ** 31, "the single vector is not strided: no workgroup counts a second chunk"
    return n


def select_group_sizes(c) -> list:
    """Three lengths that share more than target x chunk values unequally: every one of them is strided."""
    base = c["select_grid_target"] * c["select_chunk_values"]
    chunk = c["select_chunk_values"]
    lengths = [int(0.70 * base) + 3 * chunk + 11, int(0.30 * base) + 2 * chunk + 5, int(0.02 * base) + chunk + 3]
    for order in (lengths, lengths[::-1]):
        for blocks, chunks in select_blocks(order, c):
            assert blocks < chunks, "a vector of the group is not strided"
    return lengths


def select_second_turn_first_value(n: int, n_group_total: int, c) -> int:
    """The first value a workgroup of this vector reads in its second turn: chunk number `blocks`."""
    share = int(float(c["select_grid_target"]) * float(n) / float(n_group_total)) + 1
    return share * c["select_chunk_values"]


def select_vector(n: int, seed: int, low_from: int, low_to: int) -> np.ndarray:
    """n seeded normal values rounded to two decimals (ties), one in seven 0.0, a few +-inf and -0.0 near its head.  The values of
    [low_from, low_to) lie 1000 lower than all others: they alone hold the lowest ranks and the mass below every other
    rank, so leaving their turn out, or counting it twice, moves every wanted rank."""
    rng = np.random.default_rng(seed)
    x = np.round(rng.normal(0.0, 3.0, size=n), 2) + 0.0
    x[::7] = 0.0
    x[low_from:low_to] -= 1000.0
    for k, value in enumerate((np.inf, -np.inf, -0.0, np.inf, -0.0, -np.inf, -0.0)):
        x[1001 + 7919 * k] = value
    return x


def order_keys(v: np.ndarray) -> np.ndarray:
    """The select's order-preserving keys (`locus_summaries_cases.key_sorted` sorts by the same)."""
    bits = v.view(np.uint64)
    keys = np.where(bits >> np.uint64(63) != 0, ~bits, bits | np.uint64(1 << 63))
    return np.where(np.isnan(v), np.uint64(0xFFFFFFFFFFFFFFFF), keys)


def select_expected_bits(x: np.ndarray, ranks, mode: int = 0, center: float = 0.0) -> list:
    """The bit patterns `NumpyVector(x).select(ranks, mode, center)` has (a NaN as the select returns it, 0x7FFF...F), from
    one np.partition of the keys instead of a full sort; tests/test_launch_turns_sizes.py holds the two against each other."""
    with np.errstate(all="ignore"):
        v = x if mode == 0 else np.where(np.isfinite(x), np.abs(x - center), np.nan)
    keys = order_keys(np.ascontiguousarray(v, dtype=np.float64))
    wanted = sorted({int(r) for r in ranks})
    part = np.partition(keys, wanted)
    out = []
    for r in ranks:
        key = int(part[int(r)])
        out.append(key ^ (1 << 63) if key >> 63 else (~key) & 0xFFFFFFFFFFFFFFFF)
    return out


def spread_ranks(n: int, below: int, k: int = 16) -> list:
    """k ranks: four inside the lowest `below` (the values only one turn holds), the others spread over the vector."""
    low = [0, below // 3, below // 2, below - 1]
    return low + sorted({int(r) for r in np.linspace(below, n - 1, k - len(low))})


# ---- Benjamini-Hochberg ------------------------------------------------------------------------------------------------
def bh_size(c) -> int:
    m = c["bh_max_grid"] * c["bh_threads"] + 1000
    second_turn(m, c["bh_threads"], c["bh_max_grid"])
    return m


def bh_pvalues(m: int, passing, n_nan: int, fdr: float, seed: int) -> np.ndarray:
    """m p-values, shuffled, of which the last n_nan are sign-set NaNs (they lead the device sort's output) and the others,
    in ascending order, lie just above their threshold fdr * (k + 1) / m -- they fail -- except the ranks in `passing`,
    which lie on it."""
    live = m - n_nan
    k = np.arange(live)
    p = float(fdr) * ((k + 1) / float(m)) * (1.0 + 1.0e-7)
    passing = np.asarray(passing, dtype=np.int64)
    p[passing] = float(fdr) * ((passing + 1) / float(m))
    assert np.all(np.diff(p) > 0)
    p = np.concatenate([p, -np.abs(np.full(n_nan, np.nan))])
    assert np.signbit(p[live:]).all()
    return p[np.random.default_rng(seed).permutation(m)]


def bh_mask_numpy(p: np.ndarray, fdr: float) -> np.ndarray:
    """The procedure as NumPy states it on the host: ascending p (np.argsort has every NaN last), rank k passes when
    p_(k) <= fdr * (k + 1) / m, everything up to the last passing rank is taken."""
    m = p.shape[0]
    order = np.argsort(p, kind="stable")
    passed = np.flatnonzero(p[order] <= float(fdr) * (np.arange(1, m + 1) / float(m)))
    mask = np.zeros(m, dtype=bool)
    if passed.size:
        mask[order[: int(passed.max()) + 1]] = True
    return mask


# ---- records -----------------------------------------------------------------------------------------------------------
def plain_records(n: int, seed: int, spacing: int = 10, first: int = 100):
    """n records on ascending positions, spans of 50, both strands, every one passing the usual filters: the six arrays."""
    rng = np.random.default_rng(seed)
    pos = (first + spacing * np.arange(n, dtype=np.int64) + rng.integers(0, spacing, size=n)).astype(np.int32)
    flag = np.where(rng.random(n) < 0.5, 0, 16).astype(np.uint16)
    return [pos, (pos + 50).astype(np.int32), np.zeros(n, np.int32), flag, np.full(n, 30, np.uint8), np.ones(n, np.uint8)]


def chrom_range_size(c) -> int:
    n = c["chrom_range_max_grid"] * c["count_threads"] + 3000
    second_turn(n, c["count_threads"], c["chrom_range_max_grid"])
    return n


def chrom_range_case(c, in_second_turn: bool):
    """(fields, chrom_size, flag_exclude, the indices of the passing records): flag_exclude passes only the records of one
    stretch, which lies wholly in the second turn or wholly in the first; their ends are ragged, so the end of the LAST
    passing record is not the largest."""
    n = chrom_range_size(c)
    turn = c["chrom_range_max_grid"] * c["count_threads"]
    fields = plain_records(n, 41)
    rng = np.random.default_rng(42)
    fields[1] = (fields[0] + rng.integers(1, 400, size=n)).astype(np.int32)
    lo, hi = (turn + 700, n - 900) if in_second_turn else (300, turn - 500)
    excluded = np.ones(n, dtype=bool)
    excluded[lo:hi] = False
    excluded[lo + 1: hi - 1][rng.random(hi - lo - 2) < 0.5] = True
    fields[3] = (fields[3] | np.where(excluded, 1024, 0)).astype(np.uint16)
    chrom_size = int(fields[0][-1]) + 1000  # (every record reaches into the last 2 Mb or none but the last do)
    return tuple(fields), chrom_size, 1024, np.flatnonzero(~excluded)


def count_tail_size(c) -> int:
    n = c["count_tail_max_grid"] * c["count_threads"] + 5 * c["count_threads"] + 77
    second_turn(n, c["count_threads"], c["count_tail_max_grid"])
    return n


def count_tail_counts(c, where: str) -> np.ndarray:
    """float32 counts over more bins than one turn takes, positive only in the second turn ("second"), only in the first
    ("first"), or in both ("both")."""
    n = count_tail_size(c)
    turn = c["count_tail_max_grid"] * c["count_threads"]
    rng = np.random.default_rng(51)
    counts = np.zeros(n, dtype=np.float32)
    if where in ("second", "both"):
        at = turn + 33 + np.flatnonzero(rng.random(n - turn - 60) < 0.4)
        counts[at] = rng.integers(1, 5000, size=at.size)
    if where in ("first", "both"):
        at = 37 + np.flatnonzero(rng.random(5000) < 0.4)
        counts[at] = rng.integers(1, 5000, size=at.size)
    return counts


def interval_facts_size(c) -> int:
    n = c["interval_facts_max_grid"] * c["count_intervals_threads"] + 3 * c["count_intervals_threads"] + 41
    second_turn(n, c["count_intervals_threads"], c["interval_facts_max_grid"])
    return n


def interval_long_record_case(c, in_second_turn: bool):
    """(fields, the long record's index, an interval only that record reaches): one span of 5000 among spans of 50, a gap of
    6000 behind it."""
    n = interval_facts_size(c)
    turn = c["interval_facts_max_grid"] * c["count_intervals_threads"]
    at = turn + 300 if in_second_turn else 1000
    fields = plain_records(n, 61)
    pos = fields[0].astype(np.int64)
    pos[at + 1:] += 6000
    fields[0] = pos.astype(np.int32)
    end = pos + 50
    end[at] = pos[at] + 5000
    fields[1] = end.astype(np.int32)
    fields[3][at] = 0
    start = int(pos[at]) + 3000
    assert pos[at + 1] > start + 10 and end[at - 1] < start
    return tuple(fields), at, (start, start + 10)


def interval_descent_case(c):
    """The fields of a track whose only descent in pos lies in the second turn."""
    n = interval_facts_size(c)
    at = c["interval_facts_max_grid"] * c["count_intervals_threads"] + 100
    fields = plain_records(n, 62)
    fields[0][at] = fields[0][at - 1] - 3
    assert np.flatnonzero(np.diff(fields[0].astype(np.int64)) < 0).tolist() == [at - 1]
    return tuple(fields), at


def flag_facts_sizes(c) -> list:
    n = c["fragment_max_grid"] * c["fragment_threads"] + 333
    total = n + 500
    second_turn(total, c["fragment_threads"], c["fragment_max_grid"])
    assert n % 64 != 0 and n > c["fragment_max_grid"] * c["fragment_threads"], "no wavefront of the second turn straddles the tracks"
    return [n, 0, 500]


def flag_facts_case(c, descent: bool):
    """Three tracks (the middle one empty) of seven arrays; some records unmapped.  The last pos of the first track exceeds
    the first of the third.  descent: the first track's only descent at index cap x threads + 100."""
    sizes = flag_facts_sizes(c)
    rng = np.random.default_rng(71)
    tracks = []
    for k, n in enumerate(sizes):
        f = plain_records(n, 72 + k)
        f[3] = (f[3] | np.where(rng.random(n) < 0.07, 4, 0)).astype(np.uint16)
        tracks.append(f)
    if descent:
        at = c["fragment_max_grid"] * c["fragment_threads"] + 100
        tracks[0][0][at] = tracks[0][0][at - 1] - 1
    assert int(tracks[0][0][-1]) > int(tracks[2][0][0])
    return [tuple(f) for f in tracks]


def template_size(c) -> int:
    n = c["fragment_max_grid"] * c["fragment_threads"] + 100 + 3000
    second_turn(n + 700, c["fragment_threads"], c["fragment_max_grid"])
    return n


def template_file(c, in_second_turn: bool):
    """A paired-end file as tests/fragment_length_expected.py takes it, (contigs, {name: seven arrays}): contig a holds
    template_size records of which only 3000 -- those behind the first cap x threads + 100 records, or the first 3000 -- carry
    the proper-pair flag; contig b, shorter, holds 700 more.  Fewer than 2000 of a's qualify, so b's are read too."""
    n = template_size(c)
    rng = np.random.default_rng(81)

    def records(count, seed, proper):
        f = plain_records(count, seed)
        flag = f[3].astype(np.int64) | 1 | np.where(rng.random(count) < 0.5, 64, 128)
        flag |= np.where(proper, 2, 0) | np.where(rng.random(count) < 0.1, 8, 0) | np.where(rng.random(count) < 0.1, 1024, 0)
        isize = rng.integers(-1400, 1400, size=count).astype(np.int32)
        mate_same = (rng.random(count) < 0.9).astype(np.uint8)
        return dict(pos=f[0], end=f[1], isize=isize, flag=flag.astype(np.uint16), mapq=f[4], mate_same=mate_same,
                    qlen=np.full(count, 50, dtype=np.int32))

    proper = np.zeros(n, dtype=bool)
    if in_second_turn:
        proper[n - 3000:] = True
    else:
        proper[:3000] = True
    a = records(n, 82, proper)
    b = records(700, 83, np.ones(700, dtype=bool))
    contigs = [("a", int(a["pos"][-1]) + 1000), ("b", int(b["pos"][-1]) + 1000)]
    return contigs, {"a": a, "b": b}


def density_size(c) -> int:
    n = c["fragment_max_grid"] * c["fragment_density_records"] + 3 * c["fragment_density_records"] + 517
    second_turn(n, c["fragment_density_records"], c["fragment_max_grid"])
    return n


DENSITY_CHUNK = 250  # rolling_chunk_size of the density case
DENSITY_BLOCK = 5000


def density_case(c):
    """(pos, flag, contig length, flag_exclude, the first record of the second turn): records spread 10 bp apart over the
    first turn; the second turn begins inside a pile of 3000 records on 200 bp -- the densest place of the contig, so the
    first centre comes from it -- and goes on with records 1500 bp apart, which leave the LDS window of their trip
    (density_window cells of 250 bp behind its first cell).  The first turn has a sparse stretch of its own."""
    n = density_size(c)
    turn = c["fragment_max_grid"] * c["fragment_density_records"]
    rng = np.random.default_rng(91)
    step = np.full(n, 10, dtype=np.int64)
    step[200000:203000] = 1500                      # sparse, first turn
    step[turn - 800: turn + 2200] = 0               # the pile: begins before the turn's end, ends in the second turn
    step[turn - 800: turn + 2200][::15] = 1
    step[turn + 2200:] = 1500                       # sparse, second turn
    pos = 1000 + np.cumsum(step)
    assert 1500 * c["fragment_density_records"] > DENSITY_CHUNK * c["fragment_density_window"], "the sparse records stay inside the window"
    flag = (np.where(rng.random(n) < 0.5, 16, 0) | np.where(rng.random(n) < 0.05, 4, 0) | np.where(rng.random(n) < 0.05, 1024, 0))
    contig_length = int(pos[-1]) + 777
    assert contig_length < 2 ** 31
    return pos.astype(np.int32), flag.astype(np.uint16), contig_length, 1024, turn


# ---- the BAM stream ----------------------------------------------------------------------------------------------------
BAM_CONTIGS = [("c1", 2 ** 30), ("c2", 2 ** 30), ("c3", 2 ** 30)]
BAM_RECORD = np.dtype([("block_size", "<i4"), ("tid", "<i4"), ("pos", "<i4"), ("l_read_name", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                       ("n_cigar", "<u2"), ("flag", "<u2"), ("l_seq", "<i4"), ("mtid", "<i4"), ("mpos", "<i4"), ("isize", "<i4"),
                       ("name", "S4"), ("cigar", "<u4", (3,)), ("seq", "u1", (2,)), ("qual", "u1", (4,)), ("tags", "u1", (14,))])
BAM_LENGTHS = (60, 64, 68, 72)  # bytes of a record, its block_size word included


def bam_sizes(c) -> dict:
    # (16 / 15 = 64 / 60: were every record of the shortest length, the stream would still hold more than cap x threads segments of 64 bytes)
    n = c["bam_max_grid"] * c["bam_threads"] * 16 // 15 + 3 * c["bam_threads"] + 19
    turn = second_turn(n, c["bam_threads"], c["bam_max_grid"])  # bam_fields_kernel: records
    least_bytes = n * min(BAM_LENGTHS)
    # bam_walk_kernel and bam_emit_kernel at S = 64: more segments than cap x threads whatever lengths are drawn, fewer than twice
    assert least_bytes // 64 > c["bam_max_grid"] * c["bam_threads"] and (n * max(BAM_LENGTHS) + 1024) // 64 < 2 * c["bam_max_grid"] * c["bam_threads"]
    # bam_guess_kernel at S = 4096: past its cap of one segment per workgroup, the walk inside its first turn
    assert c["bam_max_grid"] < least_bytes // 4096 and (n * max(BAM_LENGTHS) + 1024) // 4096 < c["bam_max_grid"] * c["bam_threads"]
    return {"records": n, "first_record_of_second_turn": turn}


@functools.lru_cache(maxsize=1)
def bam_stream(n: int, seed: int = 101):
    """(stream bytes as a uint8 array, entry0, offsets, {field: expected array}) of n well-formed records of seeded lengths
    60 / 64 / 68 / 72 bytes on three contigs, the last 1500 without a contig, behind a header.  Every record: a name of four
    bytes, the CIGAR aM dN (4 - a)M, l_seq = 4, and tag bytes to its length."""
    assert BAM_RECORD.itemsize == max(BAM_LENGTHS)
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=BAM_RECORD)
    length = rng.choice(np.asarray(BAM_LENGTHS), size=n)
    unplaced = np.arange(n) >= n - 1500
    tid = np.where(unplaced, -1, np.minimum(np.arange(n) * 3 // (n - 1500), 2)).astype(np.int32)
    pos = np.zeros(n, dtype=np.int64)
    for k in range(3):
        mine = tid == k
        pos[mine] = 5 + np.cumsum(rng.integers(0, 40, size=int(mine.sum())))
    pos[unplaced] = -1
    flag = np.where(rng.random(n) < 0.5, 0, 16) | np.where(rng.random(n) < 0.3, 1 | 2 | 64, 0) | np.where(rng.random(n) < 0.04, 4, 0)
    flag = np.where(unplaced, 4 | (flag & 16), flag)
    a, d = rng.integers(1, 4, size=n), rng.integers(0, 1200, size=n)
    mtid = np.where(rng.random(n) < 0.8, tid, rng.integers(-1, 3, size=n)).astype(np.int32)
    rec["block_size"], rec["tid"], rec["pos"] = length - 4, tid, pos
    rec["l_read_name"], rec["mapq"], rec["bin"] = 4, rng.integers(0, 61, size=n), 4680
    rec["n_cigar"], rec["flag"], rec["l_seq"], rec["mtid"], rec["mpos"] = 3, flag, 4, mtid, -1
    rec["isize"] = rng.integers(-900, 900, size=n)
    rec["name"] = b"rd1"
    rec["cigar"] = np.stack([(a << 4) | 0, (d << 4) | 3, ((4 - a) << 4) | 0], axis=1)
    rec["seq"], rec["qual"], rec["tags"] = 0x11, 0xFF, 0x7F
    rows = rec.view(np.uint8).reshape(n, BAM_RECORD.itemsize)
    header = np.frombuffer(bx.make_header(BAM_CONTIGS, "@HD"), dtype=np.uint8)  # (48 bytes: one record start in sixteen lies on a segment's first byte)
    data = np.concatenate([header, rows[np.arange(BAM_RECORD.itemsize)[None, :] < length[:, None]]])
    entry0 = int(header.size)
    offsets = entry0 + np.concatenate([[0], np.cumsum(length)[:-1]]).astype(np.int64)
    assert data.size == entry0 + int(length.sum()) and entry0 % 4 == 0 and np.count_nonzero(offsets % 64 == 0) > n // 32
    rlen = np.where(flag & 4, 0, 4 + d)
    want = dict(tid=tid, pos=pos.astype(np.int32), end=(pos + np.where(rlen == 0, 1, rlen)).astype(np.int32), isize=rec["isize"].astype(np.int32),
                flag=flag.astype(np.uint16), mapq=rec["mapq"].astype(np.uint8), mate_same=(mtid == tid).astype(np.uint8),
                qlen=np.full(n, 4, dtype=np.int32))
    return data, entry0, offsets, want


def bam_true_entries(offsets: np.ndarray, n_bytes: int, segment_bytes: int) -> np.ndarray:
    """`bam_expected.true_entries` from the offsets: the first record start of every segment, -1 where there is none."""
    out = np.full(max(-(-n_bytes // segment_bytes), 1), -1, dtype=np.int64)
    segment, first = np.unique(offsets // segment_bytes, return_index=True)
    out[segment] = offsets[first]
    return out


def bam_sample_agrees_with_the_sequential_statement(data, entry0, offsets, want, lo: int, hi: int) -> None:
    """Records lo .. hi - 1 of the stream, cut out as a stream of their own: `bam_expected.walk`, `fields` and `true_entries`
    give what the construction says, and the first of them is `bam_expected.make_record`'s bytes."""
    begin, end = int(offsets[lo]), int(offsets[hi]) if hi < offsets.size else int(data.size)
    piece = data[begin:end].tobytes()
    walked, behind, why, where = bx.walk(piece, 0)
    assert (behind, why, where) == (len(piece), 0, -1) and np.array_equal(walked, offsets[lo:hi] - begin)
    got, first_error = bx.fields(piece, walked, len(BAM_CONTIGS))
    assert first_error == (0, -1)
    for name, _ in bx.FIELDS:
        assert np.array_equal(got[name], want[name][lo:hi]), name
    assert np.array_equal(bx.true_entries(piece, 0, 64), bam_true_entries(walked, len(piece), 64))
    size = int(offsets[lo + 1] - offsets[lo])
    words = struct.unpack_from("<3I", piece, 40)
    made = bx.make_record(size, tid=int(want["tid"][lo]), pos=int(want["pos"][lo]), flag=int(want["flag"][lo]), mapq=int(want["mapq"][lo]),
                          name=b"rd1\0", cigar=[(w & 15, w >> 4) for w in words], l_seq=4, mtid=struct.unpack_from("<i", piece, 24)[0],
                          mpos=-1, isize=int(want["isize"][lo]))
    assert made == piece[:size]
