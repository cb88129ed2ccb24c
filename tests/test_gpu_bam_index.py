"""GPU: contigs of BAM files read through their ``.bai`` indexes (note (32)):
`rocco_amd.bam.read_alignment_spans` against the whole-file read and htslib's iterator dump on the indexes htslib wrote
(tests/golden/bam_index.npz); the seams between streams on synthetic files whose blocks and records are cut where the test
chooses (tests/bam_index_files.py); `rocco_hip_bam_stream_firsts` alone against ``np.searchsorted``; indexes that lie; the
launches of a group; the routing of the reference-signature entry points through the index; the per-contig cache."""
import logging
import os

import numpy as np
import pytest

import bam_expected as bx
import bam_index_files as bif
import bam_matrix_cases as mx

pytestmark = pytest.mark.gpu

FILES = ["mixed", "blocks", "longread", "header_only", "one_record", "unplaced_only", "decoy", "wide", "shared", "edges"]
FIELDS = ("pos", "end", "isize", "flag", "mapq", "mate_same", "qlen")
S = 64  # segment_bytes of the seam tests


@pytest.fixture(scope="module")
def indexed(tmp_path_factory):
    from rocco_amd import bam

    root = tmp_path_factory.mktemp("bam_index")
    bam.clear_alignment_cache()
    yield {key: bif.write_indexed(root, key) for key in FILES + ["cg"]}
    bam.clear_alignment_cache()


@pytest.fixture(scope="module")
def whole(indexed, gpu):
    """Every fixture file through the whole-file read, once: {key: AlignmentFileRecords}."""
    from rocco_amd import bam

    return {key: bam.read_alignment_file(indexed[key])[0] for key in FILES}


def same(a, b) -> bool:
    import torch

    return all(getattr(a, f).dtype == getattr(b, f).dtype and getattr(a, f).device == getattr(b, f).device and torch.equal(getattr(a, f), getattr(b, f)) for f in FIELDS)


def host(records) -> dict:
    out = {f: getattr(records, f).cpu().numpy() for f in FIELDS}
    out["flag"] = out["flag"].view(np.uint16)
    return out


# ---- 1. parity with the whole-file read and with htslib's iterator --------------------------------------------------------
@pytest.mark.parametrize("inflate", ["host", "device"])
@pytest.mark.parametrize("key", FILES)
def test_every_contig_equals_the_whole_file_read_and_htslibs_iterator(gpu, indexed, whole, key, inflate):
    from rocco_amd import bam

    arrays, meta = bif.golden()
    if key in meta["new_files"]:  # (no htslib dump of the new files' fields: the NumPy statement, itself pinned to htslib's dumps)
        data, _ = bx.inflate(bif.golden_bam(key))
        offsets, _, _, _ = bx.walk(data, bx.header(data)[2])
        dump, _ = bx.fields(data, offsets, len(meta["files"][key]["contigs"]))
    else:
        dump = bx.dump(key)
    for t, (contig, _) in enumerate(meta["files"][key]["contigs"]):
        (got,) = bam.read_alignment_spans([(indexed[key], contig)], inflate=inflate)
        assert same(got, whole[key].records[contig]), (key, contig)
        ordinals = arrays[f"itr_{key}_{t}"]
        assert len(got) == ordinals.size == meta["files"][key]["refs"][t]["records"]
        mine = host(got)
        for f in FIELDS:
            assert np.array_equal(mine[f], dump[f][ordinals].astype(mine[f].dtype)), (key, contig, f)
    with pytest.raises(KeyError, match="no contig chrQ"):
        bam.read_alignment_spans([(indexed[key], "chrQ")], inflate=inflate)


def test_the_cg_record_is_reported_with_file_and_contig(gpu, indexed):
    from rocco_amd import bam

    with pytest.raises(ValueError, match=r"cg\.bam: contig chrA: record \d+ of the contig, at byte \d+ of its span: .*CG tag"):
        bam.read_alignment_spans([(indexed["cg"], "chrA")])
    assert [len(r) for r in bam.read_alignment_spans([(indexed["cg"], "chrB"), (indexed["cg"], "chrC")])] == [0, 0]


@pytest.mark.parametrize("inflate", ["host", "device"])
def test_batched_reads_give_the_same_arrays(gpu, indexed, whole, inflate):
    """All contigs of a file in one call; one contig of all files in one call (the files of three and of five contigs fall
    into groups of their own); a mixed list with contigs out of header order."""
    from rocco_amd import bam

    _, meta = bif.golden()
    for key in ("mixed", "shared", "edges", "wide"):
        names = [c for c, _ in meta["files"][key]["contigs"]]
        got = bam.read_alignment_spans([(indexed[key], c) for c in names], inflate=inflate)
        assert all(same(g, whole[key].records[c]) for g, c in zip(got, names)), key
    for contig in ("chrA", "chrC"):
        got = bam.read_alignment_spans([(indexed[key], contig) for key in FILES], inflate=inflate)
        assert all(same(g, whole[key].records[contig]) for g, key in zip(got, FILES)), contig
    wanted = [("shared", "chrC"), ("shared", "chrB"), ("mixed", "chrA"), ("shared", "chrD"), ("edges", "chrE"), ("shared", "chrD"), ("wide", "chrB")]
    got = bam.read_alignment_spans([(indexed[k], c) for k, c in wanted], inflate=inflate)
    assert all(same(g, whole[k].records[c]) for g, (k, c) in zip(got, wanted))
    assert bam.read_alignment_spans([], inflate=inflate) == []


# ---- 2. seams ----------------------------------------------------------------------------------------------------------------
SEAM_CONTIGS = [("e0", 1000), ("a", 100000), ("e1", 1000), ("b", 100000), ("c", 100000), ("one", 100000), ("e2", 1000)]


def seam_file(root, name, a_sizes, b_sizes=(200, 40, 64), cuts=None):
    """e0 (empty), a, e1 (empty), b (begins with a record longer than a segment), c, one (one record), e2 (empty)."""
    records = [(1, n) for n in a_sizes] + [(3, n) for n in b_sizes] + [(4, 50), (4, 78), (4, 64)] + [(5, 44)]
    total = sum(n for _, n in records)
    cuts = cuts if cuts is not None else [sum(a_sizes) - 20, sum(a_sizes) + 30, total - 90]
    return bif.write_pair(root, name, bif.synthetic_bam(SEAM_CONTIGS, records, cuts=cuts, tail=2))


@pytest.fixture(scope="module")
def seams(tmp_path_factory, gpu):
    """Three files whose contig `a` holds 128, 127 and 129 bytes: laid first, the seam behind it falls exactly on a segment
    boundary of 64 bytes, one byte before it and one byte after it.  {name: (path, whole-file records)}."""
    from rocco_amd import bam

    root = tmp_path_factory.mktemp("seams")
    out = {}
    for name, a_sizes in (("on", (64, 64)), ("before", (64, 63)), ("after", (64, 65))):
        path = seam_file(root, name, a_sizes)
        out[name] = (path, bam.read_alignment_file(path)[0])
    return out


@pytest.mark.parametrize("inflate", ["host", "device"])
@pytest.mark.parametrize("name", ["on", "before", "after"])
def test_seams_on_and_around_a_segment_boundary(gpu, seams, name, inflate):
    """Streams of zero records first, between and last, a stream of one record, a record longer than a segment right behind
    the seam; the same list split into three groups, and with a budget so small that `b` takes the slab loop."""
    from rocco_amd import bam

    path, want = seams[name]
    order = ["e0", "a", "e1", "b", "c", "one", "e2"]
    for wanted in (order, ["a", "b"], ["e0"], ["one"], ["a"], ["e1", "e2"], ["a", "a", "c", "c"]):
        got = bam.read_alignment_spans([(path, c) for c in wanted], inflate=inflate, segment_bytes=S)
        assert all(same(g, want.records[c]) for g, c in zip(got, wanted)), (name, wanted)
        assert [len(g) for g in got] == [len(want.records[c]) for c in wanted]
    assert [len(want.records[c]) for c in ("a", "b", "c", "one", "e0")] == [2, 3, 3, 1, 0]
    calls, slabs = [], []
    walk, decode = bam.walk_records_device, bam.decode_records_device
    bam.walk_records_device = lambda *a, **kw: (calls.append(int(a[0].shape[0])), walk(*a, **kw))[1]
    bam.decode_records_device = lambda *a, **kw: (slabs.append(int(a[0].shape[0])), decode(*a, **kw))[1]
    try:
        # a: about 128 bytes, b: 304, c: 192, one: 44.  Three groups either way: (e0, a, e1), (b), (c, one, e2); under the smaller
        # budget b alone exceeds it and is read by the slab loop, entered behind the bytes of `a` that share its first block
        for budget, by_slabs in ((320, 0), (250, 1)):
            del calls[:], slabs[:]
            got = bam.read_alignment_spans([(path, c) for c in order], inflate=inflate, segment_bytes=S, batch_bytes=budget)
            assert all(same(g, want.records[c]) for g, c in zip(got, order)), (name, budget)
            assert len(calls) == 3 and (len(slabs) >= 1) == bool(by_slabs), (budget, calls, slabs)
    finally:
        bam.walk_records_device, bam.decode_records_device = walk, decode


@pytest.mark.parametrize("K", [1, 70])
def test_one_contig_of_k_files_in_one_group(gpu, seams, K, monkeypatch):
    from rocco_amd import bam

    names = ["on", "before", "after"]
    wanted = [(seams[names[k % 3]][0], "abc"[k % 2]) for k in range(K)]  # (contigs a, b, a, b, ...: each file's own)
    wanted = sorted(wanted, key=lambda pair: pair[1])  # reference ids must not descend within a group
    walks = []
    walk = bam.walk_records_device
    monkeypatch.setattr(bam, "walk_records_device", lambda *a, **kw: (walks.append(1), walk(*a, **kw))[1])
    for inflate in ("host", "device"):
        del walks[:]
        got = bam.read_alignment_spans(wanted, inflate=inflate, segment_bytes=S)
        assert len(got) == K and len(walks) == 1
        for g, (path, contig) in zip(got, wanted):
            assert same(g, next(w for p, w in seams.values() if p == path).records[contig])


def test_a_long_stream_takes_the_slab_loop(gpu, indexed, whole):
    """`wide` chrA spans several BGZF blocks of htslib's own size: with a budget below it, it is read slab by slab, the
    slabs cut at block boundaries, the first entered at the span's begin and the last cut at its end."""
    from rocco_amd import bam

    for inflate in ("host", "device"):
        slabs = []
        decode = bam.decode_records_device
        bam.decode_records_device = lambda *a, **kw: (slabs.append(1), decode(*a, **kw))[1]
        try:
            got = bam.read_alignment_spans([(indexed["wide"], c) for c in ("chrB", "chrA", "chrD", "chrC")], inflate=inflate, batch_bytes=40000)
        finally:
            bam.decode_records_device = decode
        assert all(same(g, whole["wide"].records[c]) for g, c in zip(got, ("chrB", "chrA", "chrD", "chrC")))
        assert len(slabs) >= 3


# ---- 3. rocco_hip_bam_stream_firsts alone -----------------------------------------------------------------------------------
def made_up(n, K, seed, empty=()):
    """(offsets, tid, bounds, expect): n ascending offsets, K streams whose bounds are record starts; ``empty``: streams made
    empty by repeating the bound behind them."""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(rng.integers(36, 120, size=n))]).astype(np.int64)
    n_bytes, offsets = int(offsets[-1]), offsets[:-1]
    cut = np.sort(rng.choice(np.arange(1, max(n, 2)), size=min(K - 1, max(n - 1, 0)), replace=False)) if n > 1 else np.zeros(0, dtype=np.int64)
    starts = [0] + [int(offsets[c]) for c in cut]
    while len(starts) < K:
        starts.append(n_bytes)
    bounds = np.asarray(sorted(starts) + [n_bytes], dtype=np.int64)
    for j in sorted(empty, reverse=True):  # (the first bound stays the first record: stream 0 is emptied by pulling the bound behind it down)
        bounds[j + (j == 0)] = bounds[j + 1 - (j == 0)]
    bounds = np.sort(bounds)
    expect = rng.permutation(K).astype(np.int32)
    tid = expect[np.clip(np.searchsorted(bounds[:K], offsets, side="right") - 1, 0, K - 1)] if n else np.zeros(0, dtype=np.int32)
    return offsets, tid.astype(np.int32), bounds, expect


def firsts_of(gpu, offsets, tid, bounds, expect):
    import torch

    from rocco_amd import bam

    return bam.stream_firsts_device(torch.from_numpy(offsets).to(gpu), torch.from_numpy(tid).to(gpu), bounds.tolist(), expect.tolist())


def searchsorted_firsts(offsets, bounds):
    want = np.searchsorted(offsets, bounds, side="left")
    want[-1] = offsets.size
    return want.tolist()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
@pytest.mark.parametrize("K", [1, 2, 7, 70])
def test_stream_firsts_against_searchsorted(gpu, n, K):
    offsets, tid, bounds, expect = made_up(n, K, 100 * K + n)
    firsts, error = firsts_of(gpu, offsets, tid, bounds, expect)
    assert firsts == searchsorted_firsts(offsets, bounds) and error == (0, -1)


def test_stream_firsts_with_repeated_bounds(gpu):
    """Empty streams first, in the middle (two in a row) and last: a record on a repeated bound belongs to the LAST stream
    that begins there, the streams before it are empty."""
    offsets, tid, bounds, expect = made_up(300, 9, 5, empty=(0, 3, 4, 7))
    assert np.unique(bounds).size < bounds.size
    firsts, error = firsts_of(gpu, offsets, tid, bounds, expect)
    assert firsts == searchsorted_firsts(offsets, bounds) and error == (0, -1)
    assert sum(1 for a, b in zip(firsts, firsts[1:]) if a == b) >= 4
    # all bounds equal but the last: one stream holds everything
    bounds[:] = [0] * 9 + [int(bounds[-1])]
    firsts, error = firsts_of(gpu, offsets, np.full(300, expect[8], dtype=np.int32), bounds, expect)
    assert firsts == [0] * 9 + [300] and error == (0, -1)


def test_stream_firsts_past_one_launchs_first_turn(gpu):
    """n = cap x threads + 3 (from the library's own caps): the last lanes take a second record."""
    from rocco_amd import _native

    caps = _native.launch_caps()
    n = caps["bam_max_grid"] * caps["bam_threads"] + 3
    offsets, tid, bounds, expect = made_up(n, 70, 9)
    firsts, error = firsts_of(gpu, offsets, tid, bounds, expect)
    assert firsts == searchsorted_firsts(offsets, bounds) and error == (0, -1)
    tid[n - 1] = (tid[n - 1] + 1) % 70 if expect[69] != (tid[n - 1] + 1) % 70 else (tid[n - 1] + 2) % 70
    firsts, error = firsts_of(gpu, offsets, tid, bounds, expect)  # (a wrong reference id on a second-turn record is seen)
    assert error == (13, int(np.searchsorted(bounds[:70], offsets[n - 1], side="right") - 1))


def test_stream_firsts_error_codes_and_their_order(gpu):
    from rocco_amd import bam

    offsets, tid, bounds, expect = made_up(400, 8, 11)
    stream_of = lambda r: int(np.searchsorted(bounds[:8], offsets[r], side="right") - 1)  # noqa: E731
    first5 = int(np.flatnonzero(offsets >= bounds[5])[0])
    assert stream_of(first5) == 5 and offsets[first5] == bounds[5] and stream_of(first5 + 2) == 5
    # a bound inside a record: the record it cuts off now lies in stream 4 with stream 5's id -- the lower stream is reported;
    # with the id stream 4 expects, what is left is the seam: stream 5 has records and its bound is no record start
    lying = bounds.copy()
    lying[5] += 3
    assert firsts_of(gpu, offsets, tid, lying, expect)[1] == (bam.ERR_SPAN_TID, 4)
    moved = tid.copy()
    moved[first5] = expect[4]
    assert firsts_of(gpu, offsets, moved, lying, expect)[1] == (bam.ERR_SEAM, 5)
    early = bounds.copy()
    early[5] -= 3  # (the bound falls inside the record before: stream 5's first record does not begin on it)
    assert firsts_of(gpu, offsets, tid, early, expect)[1] == (bam.ERR_SEAM, 5)
    # a record of another reference
    r = int(np.flatnonzero(offsets >= bounds[2])[0]) + 1
    assert stream_of(r) == 2
    wrong = tid.copy()
    wrong[r] = expect[3]
    assert firsts_of(gpu, offsets, wrong, bounds, expect)[1] == (bam.ERR_SPAN_TID, 2)
    # the lowest (stream, code) wins: a seam error in stream 5 and a wrong id in stream 2; both in stream 5
    wrong[first5] = expect[4]
    assert firsts_of(gpu, offsets, wrong, lying, expect)[1] == (bam.ERR_SPAN_TID, 2)
    moved[first5 + 2] = expect[0]
    assert firsts_of(gpu, offsets, moved, lying, expect)[1] == (bam.ERR_SEAM, 5)
    # bytes of a stream in which no record begins: the chain crossed it inside a record
    lying = np.insert(bounds, 4, bounds[4] - 5)
    assert firsts_of(gpu, offsets, tid, lying, np.insert(expect, 3, expect[3]))[1][0] == bam.ERR_SEAM
    # the first bound is not the first record; the last bound is not the stream's end
    assert firsts_of(gpu, offsets + 4, tid, bounds + np.r_[0, [4] * 8], expect)[1] == (bam.ERR_SEAM, 0)
    with pytest.raises(ValueError, match="rocco_hip_bam_stream_firsts: invalid argument"):
        firsts_of(gpu, offsets, tid, bounds[::-1].copy(), expect)  # (descending bounds are refused by the entry)


# ---- 4. a lying index ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def liars(tmp_path_factory):
    """One synthetic file (three contigs of records with real lengths, several blocks) under indexes that do not describe it."""
    root = tmp_path_factory.mktemp("liars")
    records = [(0, 60 + (k % 7)) for k in range(40)] + [(1, 90 + (k % 5)) for k in range(30)] + [(2, 50 + (k % 11)) for k in range(25)]
    raw = bif.synthetic_bam([("c0", 100000), ("c1", 100000), ("c2", 100000)], records, cuts=(700, 2000, 3100, 4400), tail=3)
    facts = bif.facts(raw)
    refs, n_no_coor = bif.build_index(raw)
    table, v, tid = facts["blocks"], facts["voffsets"], facts["fields"]["tid"]
    inside = lambda r, k: bif.voffset(table, len(raw), int(facts["offsets"][r]) + k)  # noqa: E731

    def with_pseudo(changes):
        out = [dict(ref) for ref in refs]
        for t, pseudo in changes.items():
            out[t]["pseudo"] = pseudo
        return bif.bai_bytes(out, n_no_coor)

    first = [int(np.flatnonzero(tid == t)[0]) for t in range(3)]
    last = [int(np.flatnonzero(tid == t)[-1]) for t in range(3)]
    p = [ref["pseudo"] for ref in refs]
    other = bif.synthetic_bam([("c0", 100000), ("c1", 100000), ("c2", 100000)], [(0, 4000), (1, 3000), (1, 2500), (2, 64)], cuts=(3000, 6000))
    cases = {
        "end_inside": with_pseudo({1: (p[1][0], inside(last[1], 13)) + p[1][2:]}),
        "end_short": with_pseudo({0: (p[0][0], inside(last[0] - 2, 5)) + p[0][2:]}),
        "begin_inside": with_pseudo({1: (inside(first[1], 7), p[1][1]) + p[1][2:]}),
        "begin_late": with_pseudo({2: (inside(first[2] + 1, 36), p[2][1]) + p[2][2:]}),
        "swapped": with_pseudo({0: p[2], 2: p[0]}),
        "another_file": bif.index_bytes(other),
    }
    return {name: bif.write_pair(root / name if (root / name).mkdir() is None else root, "lied", raw, bai=bai) for name, bai in cases.items()}


@pytest.mark.parametrize("inflate", ["host", "device"])
@pytest.mark.parametrize("case", ["end_inside", "end_short", "begin_inside", "begin_late", "swapped", "another_file"])
def test_a_lying_index_is_a_value_error_naming_file_and_contig(gpu, liars, case, inflate):
    """Ordinary bad files: every load of the walk and of the field decode is bounded by the bytes handed over
    (csrc/bam_record.h: bam_walk_segment; bam_fields_kernel's `framed`), so a mis-framed chain ends in a report."""
    from rocco_amd import bam, bam_index

    path = liars[case]
    bam_index.clear_bam_index_cache()
    touched = {"end_inside": ["c1"], "end_short": ["c0"], "begin_inside": ["c1"], "begin_late": ["c2"], "swapped": ["c0", "c2"],
               "another_file": ["c0", "c1", "c2"]}[case]
    for contig in touched:
        with pytest.raises(ValueError) as info:
            bam.read_alignment_spans([(path, contig)], inflate=inflate, segment_bytes=S)
        assert path in str(info.value) and f"contig {contig}" in str(info.value), str(info.value)
        if case != "another_file":
            assert "does not describe this file" in str(info.value)
    with pytest.raises(ValueError) as info:  # all three in one group: the chain crosses the lied-about seam
        bam.read_alignment_spans([(path, c) for c in ("c0", "c1", "c2")], inflate=inflate, segment_bytes=S)
    assert path in str(info.value) and "contig c" in str(info.value)
    if case == "swapped":
        assert "lies on reference" in str(info.value)


# ---- 5. launches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5])
def test_one_group_costs_one_inflate_one_walk_one_field_decode(gpu, indexed, K, monkeypatch):
    from rocco_amd import bam

    counts = {"inflate_blocks_device": 0, "walk_records_device": 0, "record_fields_device": 0, "stream_firsts_device": 0}
    for name in counts:
        def counted(*a, _name=name, _real=getattr(bam, name), **kw):
            counts[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(bam, name, counted)
    keys = ["mixed", "blocks", "longread", "decoy", "one_record"][:K]
    got = bam.read_alignment_spans([(indexed[key], "chrA") for key in keys], inflate="device")
    assert len(got) == K and all(len(g) > 0 and g.pos.is_cuda and g.qlen.is_cuda for g in got)
    assert counts == {"inflate_blocks_device": 1, "walk_records_device": 1, "record_fields_device": 1, "stream_firsts_device": 1}


# ---- 6. routing ---------------------------------------------------------------------------------------------------------------
class Keep(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.DEBUG)
        self.records = []

    def emit(self, record):
        self.records.append([record.levelname, record.getMessage()])


def logged(call, paths, only=("DEBUG", "INFO", "WARNING", "ERROR")):
    from rocco_amd import bam

    keep = Keep()
    bam.logger.addHandler(keep)
    level = bam.logger.level
    bam.logger.setLevel(logging.DEBUG)
    bam._BAM_COUNT_METADATA_CACHE.clear()
    try:
        result = call()
    finally:
        bam.logger.removeHandler(keep)
        bam.logger.setLevel(level)
    log = []
    for level_name, message in keep.records:
        for key, path in paths.items():
            message = message.replace(path, "{" + key + "}")
        if level_name in only:
            log.append([level_name, message])
    return result, log


@pytest.fixture(scope="module")
def routed(tmp_path_factory):
    """Every BAM file the stored scenarios name, each with an index: htslib's for the files of bam_index.npz, the Python
    writer's (pinned to htslib) for the others."""
    from rocco_amd import bam

    root = tmp_path_factory.mktemp("routed")
    paths = mx.write_files(root)
    arrays, _ = bif.golden()
    for key, path in paths.items():
        if key == "sizes":
            continue
        with open(path, "rb") as handle:
            raw = handle.read()
        with open(path + ".bai", "wb") as handle:
            handle.write(arrays[f"bai_{key}"].tobytes() if f"bai_{key}" in arrays and bif.golden_bam(key) == raw else bif.index_bytes(raw))
    for key in ("one_record", "header_only", "decoy"):
        if key not in paths:
            paths[key] = bif.write_indexed(root, key)
    bam.clear_alignment_cache()
    yield paths
    bam.clear_alignment_cache()


@pytest.fixture()
def no_whole_file_read(monkeypatch):
    from rocco_amd import bam

    def refuse(path, *a, **kw):
        raise AssertionError(f"read_alignment_file({path}) was called: the file has an index")

    monkeypatch.setattr(bam, "read_alignment_file", refuse)
    bam.clear_alignment_cache()


def test_get_bam_chrom_reads_through_the_index(gpu, routed, no_whole_file_read):
    """The 96 stored results of the reference's get_bam_chrom_reads, none of them through a whole-file read."""
    from rocco_amd import bam

    arrays, meta = bx.golden()
    seen = 0
    for entry in meta["chrom_reads"]:
        seen += 1
        name, key = entry["name"], entry["file"]
        call = lambda: bam.get_bam_chrom_reads(routed[key], entry["contig"], routed["sizes"], entry["step"], **entry["kwargs"])
        if entry["error"] is not None:
            with pytest.raises({"RuntimeError": RuntimeError, "ValueError": ValueError}[entry["error_type"]]) as info:
                call()
            assert str(info.value).replace(routed["sizes"], "{sizes}") == entry["error"], name
            continue
        (intervals, vals), log = logged(call, routed)
        assert log == entry["log"], name
        if entry["none"]:
            assert intervals is None and vals is None, name
            continue
        want_i, want_v = arrays[f"r_{name}_intervals"], arrays[f"r_{name}_values"]
        assert intervals.dtype == want_i.dtype and np.array_equal(intervals, want_i), name
        assert vals.dtype == want_v.dtype and vals.tobytes() == want_v.tobytes(), name
    assert seen == 96
    assert all(isinstance(bam._cached_file(routed[k]), bam.IndexedAlignmentFile) for k in ("mixed", "blocks", "longread"))


def test_count_metadata_through_the_index(gpu, routed, no_whole_file_read):
    """The 8 stored dicts with their log records; the mapped reads come from the index statistics."""
    from rocco_amd import bam

    _, meta = bx.golden()
    assert len(meta["metadata"]) == 8
    for entry in meta["metadata"]:
        metadata, log = logged(lambda: bam._get_bam_count_metadata(routed[entry["file"]], **entry["call"]), routed)
        assert metadata == entry["metadata"] and log == entry["log"], entry
        assert {k: type(v) for k, v in metadata.items()} == {k: type(v) for k, v in entry["metadata"].items()}
    file = bam._cached_file(routed["mixed"])
    assert file.index_read_counts(["chrC"]) is not None and len(file.records) == 3 and "chrZ" not in file.records
    assert file.count("chrA") == len(file.records["chrA"]) == 900


def test_generate_chrom_matrix_and_run_chromosomes_through_the_index(gpu, routed, no_whole_file_read, tmp_path, monkeypatch):
    """The stored matrices of both fixture sets by their bits, with every WARNING / INFO record; the chromosome's records of
    the K files are fetched in ONE `read_alignment_spans` call; run_chromosomes writes the stored BED bytes."""
    from rocco_amd import bam
    from rocco_amd import rocco as impl

    old_arrays, old = bx.golden()
    new_arrays, new = mx.golden()
    scenarios = [(dict(r, error=None, none=False), old_arrays) for r in old["matrix"]] + [(e, new_arrays) for e in new["scenarios"]]
    fetched = []
    read = bam.read_alignment_spans
    monkeypatch.setattr(bam, "read_alignment_spans", lambda wanted, *a, **kw: (fetched.append(list(wanted)), read(wanted, *a, **kw))[1])
    for entry, arrays in scenarios:
        name = entry["name"]
        want_log = [r for r in entry["log"] if r[0] in ("WARNING", "INFO")]
        files = [routed[k] for k in entry["files"]]
        call = lambda: bam.generate_chrom_matrix_device(entry["contig"], files, routed["sizes"], entry["step"], **entry["kwargs"])
        if entry["error"] is not None:
            with pytest.raises({"RuntimeError": RuntimeError, "ValueError": ValueError}[entry["error_type"]]) as info:
                call()
            assert str(info.value).replace(routed["sizes"], "{sizes}") == entry["error"], name
            continue
        (intervals, matrix), log = logged(call, routed, only=("WARNING", "INFO"))
        assert log == want_log, name
        if entry["none"]:
            assert intervals is None and matrix is None, name
            continue
        want_i, want_m = arrays[f"{name}_intervals"], arrays[f"{name}_matrix"]
        matrix = matrix.cpu().numpy()
        assert np.array_equal(intervals, want_i) and matrix.dtype == want_m.dtype and matrix.shape == want_m.shape and \
            matrix.tobytes() == want_m.tobytes(), name
    # a fresh cache: one call fetches the chromosome of all K files at once
    bam.clear_alignment_cache()
    del fetched[:]
    record = old["matrix"][0]
    files = [routed[k] for k in record["files"]]
    bam.generate_chrom_matrix_device(record["contig"], files, routed["sizes"], record["step"], **record["kwargs"])
    assert fetched[0] == [(f, record["contig"]) for f in files]
    # the binding of INTEGRATION.md
    entries = {e["contig"]: e for e in new["scenarios"] if e["name"].startswith("all_")}
    chroms, one = ["chrA", "chrB", "chrC"], entries["chrA"]
    args = {"chrom_sizes_file": routed["sizes"], "step": one["step"], "round_digits": 5, "effective_genome_size": -1,
            "norm_method": one["kwargs"]["norm_method"], "min_mapping_score": 10, "flag_include": None, "flag_exclude": 3844,
            "extend_reads": -1, "center_reads": False, "ignore_for_norm": None, "scale_factor": 1.0, "score_lower_bound_z": 1.0,
            "score_prior_df": 6.0, "score_min_effect": None, "score_precision_floor_ratio": 0.01, "gamma": None, "budget": None,
            "scale_chrom_budgets": 1.0, "budget_posterior_quantile": 0.01, "selection_penalty": None, "min_length_bp": 100,
            "narrowPeak": False, "low_memory": False, "input_track_type": "bam", "budget_null_draws": 6,
            "threads": one["kwargs"]["num_processors"]}
    monkeypatch.chdir(tmp_path)
    from_matrices = {c: (new_arrays[f"all_{c}_intervals"], new_arrays[f"all_{c}_matrix"]) for c in chroms}
    want = impl.run_chromosomes(chroms, from_matrices, dict(args, output=str(tmp_path / "want.bed")), run_id="1")
    bam.clear_alignment_cache()
    monkeypatch.setattr(impl, "generate_chrom_matrix", bam.generate_chrom_matrix_device)
    got = impl.run_chromosomes(chroms, [routed[k] for k in one["files"]], dict(args, output=str(tmp_path / "got.bed")), run_id="2")
    with open(want, "rb") as a, open(got, "rb") as b:
        want_bytes, got_bytes = a.read(), b.read()
    assert len(want_bytes) > 0 and got_bytes == want_bytes


def test_metadata_decodes_the_leading_contigs_and_the_three_longest(gpu, tmp_path, monkeypatch):
    """A file whose first contig alone satisfies the head probes: one metadata call decodes it and, where a fragment
    length is asked for, the three longest contigs -- not the short ones behind it.  The dict equals the whole-file route's."""
    from rocco_amd import bam

    contigs = [("c0", 600000), ("c1", 500), ("c2", 9000000), ("c3", 8000000), ("c4", 7000000), ("c5", 100)]
    cigar = ((0, 30),)
    body = b"".join(bx.make_record(96, tid=0, pos=100 * k, flag=16 * (k % 2), cigar=cigar, l_seq=30) for k in range(5000))
    for tid, count in ((1, 10), (2, 60), (3, 50), (4, 40), (5, 5)):
        body += b"".join(bx.make_record(96, tid=tid, pos=40 * k, flag=16 * (k % 2), cigar=cigar, l_seq=30) for k in range(count))
    raw = bx.bgzf_compress(bx.make_header(contigs) + body)
    path = bif.write_pair(tmp_path, "long_head", raw)
    decoded = []
    read = bam.read_alignment_spans
    monkeypatch.setattr(bam, "read_alignment_spans", lambda wanted, *a, **kw: (decoded.append([c for _, c in wanted]), read(wanted, *a, **kw))[1])
    whole_reads = []
    read_file = bam.read_alignment_file
    monkeypatch.setattr(bam, "read_alignment_file", lambda p, *a, **kw: (whole_reads.append(p), read_file(p, *a, **kw))[1])
    results = {}
    for extend_reads, want in ((-1, [["c0"]]), (0, [["c0"], ["c2", "c3", "c4"]])):
        bam.clear_alignment_cache()
        del decoded[:]
        results[extend_reads] = bam._get_bam_count_metadata(path, 50, "CPM", -1, ["c5"], flag_exclude=0, extend_reads=extend_reads)
        assert decoded == want and whole_reads == []
        assert results[extend_reads]["mapped_reads"] == 5160
    # the old route: with the switch off, and for a file without an index
    monkeypatch.setattr(bam, "USE_INDEX", False)
    for extend_reads in (-1, 0):
        bam.clear_alignment_cache()
        del decoded[:]
        assert bam._get_bam_count_metadata(path, 50, "CPM", -1, ["c5"], flag_exclude=0, extend_reads=extend_reads) == results[extend_reads]
        assert decoded == [] and whole_reads == [path]
        del whole_reads[:]
    monkeypatch.setattr(bam, "USE_INDEX", True)
    bam.clear_alignment_cache()
    bare = str(tmp_path / "bare.bam")
    with open(bare, "wb") as handle:
        handle.write(raw)
    assert not isinstance(bam._cached_file(bare), bam.IndexedAlignmentFile) and whole_reads == [bare] and decoded == []
    bam.clear_alignment_cache()


# ---- 7. the cache ---------------------------------------------------------------------------------------------------------------
def test_contigs_leave_the_cache_one_by_one(gpu, indexed, monkeypatch):
    from rocco_amd import bam

    bam.clear_alignment_cache()
    file = bam._cached_file(indexed["mixed"])
    assert isinstance(file, bam.IndexedAlignmentFile) and bam._cached_file(indexed["mixed"]) is file and len(bam._ALIGNMENT_CACHE) == 0
    a = file.records["chrA"]
    assert file.records["chrA"] is a and len(bam._ALIGNMENT_CACHE) == 1  # (served from the cache)
    file.load(["chrB", "chrC", "chrA"])
    assert [key[-1] for key in bam._ALIGNMENT_CACHE] == ["chrA", "chrB", "chrC"]
    assert file.records["chrB"] is file.load(["chrB"])[0] and [key[-1] for key in bam._ALIGNMENT_CACHE] == ["chrA", "chrC", "chrB"]
    monkeypatch.setattr(bam, "ALIGNMENT_CACHE_BYTES", 20 * (500 + 150 + 1))  # room for chrB, chrC and one record more, not for chrA as well
    other = bam._cached_file(indexed["one_record"]).records["chrA"]
    assert len(other) == 1 and [key[-1] for key in bam._ALIGNMENT_CACHE] == ["chrC", "chrB", "chrA"]
    assert [key[0] for key in bam._ALIGNMENT_CACHE] == [indexed["mixed"]] * 2 + [indexed["one_record"]]
    monkeypatch.setattr(bam, "ALIGNMENT_CACHE_BYTES", 1)
    assert len(file.records["chrA"]) == 900 and [key[-1] for key in bam._ALIGNMENT_CACHE] == ["chrA"]  # (the newest entry always stays)
    assert next(iter(bam._ALIGNMENT_CACHE))[0] == indexed["mixed"]
    os.utime(indexed["mixed"], ns=(7, 7))  # a file that changes on disk is another file
    assert bam._cached_file(indexed["mixed"]) is not file
    bam.clear_alignment_cache()
    assert len(bam._ALIGNMENT_CACHE) == 0 and len(bam._INDEXED_FILES) == 0 and len(bam._BAM_COUNT_METADATA_CACHE) == 0
