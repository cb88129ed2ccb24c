"""Fragments files on the device (note (34)): the kernels of csrc/fragments_file.hip through the C
ABI against their host twin and the NumPy statement on every fixture file, both inflate modes, K sources in one group, the
structural edges of every kernel at sizes taken from `rocco_hip_fragfile_shape`, and the path functions against the
reference's stored results."""
import ctypes
import os

import numpy as np
import pytest

import fragments_expected as fx
from rocco_amd import fragments as fr, tabix_index

pytestmark = pytest.mark.gpu
META, ARRAYS = fx.load_golden()
MODES = fx.MODES
POISON = 0x5A5A5A5A


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    paths = fx.materialize(tmp_path_factory.mktemp("fragments"), META, ARRAYS)
    tabix_index.clear_tabix_index_cache()
    fr.clear_fragments_cache()
    with open(os.path.join(os.path.dirname(paths["mixed"]), "t.sizes"), "w") as handle:
        for name, length in META["sizes"].items():
            handle.write(f"{name}\t{length}\n")
        handle.write("chrX\t1000\n")
    paths["sizes"] = os.path.join(os.path.dirname(paths["mixed"]), "t.sizes")
    return paths


def source(files, key, allow="-"):
    return fr.FragmentsSource(files[key], None if allow == "-" else files["allow:" + allow])


def host(a):
    return a.cpu().numpy()


def assert_lines_equal(lines, twin, where, name_index=0):
    """``name_index``: where the lines' contig stands in the name table of the device's call (the twin's table holds it alone)."""
    for name in ("start", "end", "weight"):
        assert np.array_equal(host(getattr(lines, name)), twin[name]), (where, name)
    assert np.array_equal(host(lines.status).view(np.uint32), twin["status"]), where
    if name_index is None:
        assert np.array_equal(host(lines.name) >= 0, twin["name"] >= 0), where
    else:
        assert np.array_equal(host(lines.name), np.where(twin["name"] >= 0, name_index, -1)), where


# ---- 1. the kernels against the host twin and the reference on every fixture file ----------------------------------------

@pytest.mark.parametrize("inflate", ["host", "device"])
def test_every_span_of_every_file_against_the_host_twin(gpu, files, inflate):
    fr.clear_fragments_cache()
    pairs, twins = [], []
    for allow in ("-", "many"):
        packed = fr.load_barcode_allowlist(files["allow:many"]) if allow == "many" else fr._NO_LIST
        for key, info in META["files"].items():
            for contig in info["contigs"] + ["chrNone"]:
                pairs.append((source(files, key, allow), contig))
                text = fr.span_bytes_host(files[key], contig)
                twins.append(None if text is None else fr.fragfile_host(text, names=[contig], expect=[0], allowlists=[packed]))
    before = fr._LoadCounts.inflates
    got = fr.read_fragments_spans(pairs, device=gpu, inflate=inflate)
    # (a group ends behind a stream that ends its file: one inflate per file; the second allow-list inflates nothing)
    assert fr._LoadCounts.inflates == before + len(META["files"])
    for (src, contig), lines, twin in zip(pairs, got, twins):
        if twin is None:
            assert lines is None
            continue
        assert len(lines) == twin["lines"] > 0
        assert_lines_equal(lines, twin, (src.path, contig, src.barcode_allowlist_file), name_index=None)


def test_every_stored_count_range_and_mapped_count(gpu, files):
    """Bit for bit what the reference's counter wrote, for all four modes, both one_read_per_bin values, with and without
    allow-lists; a result beyond 2**24 is refused (there the reference's own sums depend on the order of its lines)."""
    fr.clear_fragments_cache()
    stored = [r for r in META["count"] if "error" not in r]
    lines = fr.read_fragments_spans([(source(files, r["file"], r["allow"]), r["contig"]) for r in stored], device=gpu)
    counts, maxima = fr.count_lines_batch_device(lines, [(r["start"], r["end"], r["step"]) for r in stored], [r["mode"] for r in stored],
                                                 [r["one_read_per_bin"] for r in stored], lengths=[r["length"] for r in stored], check=False)
    exact = [r for r, magnitude in zip(stored, maxima) if magnitude <= 2 ** 24]
    assert len(exact) >= 100 and 1 <= len(stored) - len(exact) <= 12
    for r, got, magnitude in zip(stored, counts, maxima):
        if magnitude <= 2 ** 24:
            assert host(got).tobytes() == ARRAYS[f"c_{r['name']}"].tobytes(), r["name"]
        elif r["length"] == ((r["end"] - r["start"] - 1) // r["step"]) + 1:
            with pytest.raises(RuntimeError, match=r"reach \d+, beyond 2\*\*24"):
                fr.count_fragments_region(source(files, r["file"], r["allow"]), r["contig"], r["start"], r["end"], r["step"], r["mode"],
                                          r["one_read_per_bin"])
    for r in META["count"]:
        if "error" in r:
            with pytest.raises(RuntimeError, match="failed to open fragments region iterator"):
                fr.count_fragments_region(files[r["file"]], r["contig"], r["start"], r["end"], r["step"])
    one = exact[3]
    got = fr.count_fragments_region(source(files, one["file"], one["allow"]), one["contig"], one["start"], one["end"], one["step"],
                                    {"cutsite": "cut", "coverage": "cov", "fiveprime": "5p", "center": "centre"}[one["mode"]], one["one_read_per_bin"])
    assert got.dtype == np.float32 and got.tobytes() == ARRAYS[f"c_{one['name']}"].tobytes()
    with pytest.raises(ValueError, match="unsupported count mode `Coverage`"):
        fr.count_fragments_region(files["plain"], "chrA", 0, 100, 10, "Coverage")
    ranges = fr.get_fragments_chrom_ranges([(source(files, r["file"], r["allow"]), r["contig"], r["chrom_len"]) for r in META["range"]])
    assert ranges == [(r["start"], r["end"]) for r in META["range"]]
    assert fr.get_fragments_chrom_range(files["mixed"], "chrC", 50000) == (777, 999)
    for inflate, slab in (("host", 1 << 26), ("device", 20000), ("host", 1)):
        for r in META["mapped"]:
            if "error" in r:
                with pytest.raises(RuntimeError, match="failed to load tabix index for fragments source"):
                    fr.get_fragments_mapped_read_count(files[r["file"]])
            elif slab > 1 or (r["file"] == "blocks" and r["allow"] == "many"):  # (a slab per block: lines carried over every seam)
                got = fr.get_fragments_mapped_read_count(source(files, r["file"], r["allow"]), r["exclude"], r["mode"], r["one_read_per_bin"],
                                                         inflate=inflate, slab_bytes=slab)
                assert got == (r["mapped"], 0), (r, inflate, slab)


def test_k_sources_in_one_group_decode_each_file_once(gpu, files):
    """Three sources over one file (three allow-lists), two other files, a contig without lines in one of them and a contig no
    index knows: one inflate and one line pass for the group, one field pass for it and one per further allow-list."""
    fr.clear_fragments_cache()
    wanted = [(source(files, "mixed"), "chrA"), (source(files, "blocks"), "chrA"), (source(files, "mixed", "many"), "chrA"),
              (source(files, "plain"), "chrB"), (source(files, "mixed", "one"), "chrA"), (source(files, "plain"), "chrA"),
              (source(files, "mixed"), "chrA")]
    before = (fr._LoadCounts.inflates, fr._LoadCounts.lines, fr._LoadCounts.fields)
    got = fr.read_fragments_spans(wanted, device=gpu)
    assert (fr._LoadCounts.inflates - before[0], fr._LoadCounts.lines - before[1], fr._LoadCounts.fields - before[2]) == (1, 1, 3)
    assert got[3] is None and got[0] is got[6] and len(got[0]) == len(got[2]) == len(got[4])
    allowed = [int((host(g.status) & fr.BARCODE_ALLOWED != 0).sum()) for g in (got[0], got[2], got[4])]
    assert allowed[0] > allowed[1] > allowed[2] > 0
    again = fr.read_fragments_spans(wanted, device=gpu, inflate="device")
    assert fr._LoadCounts.inflates - before[0] == 1 and all(a is b for a, b in zip(again, got))
    regions = [(0, 100000, 50)] * 3
    counts, _ = fr.count_lines_batch_device([got[0], got[2], got[4]], regions, ["coverage", "cutsite", "center"], [0, 0, 0])
    for k, (allow, mode) in enumerate((("-", 0), ("many", 1), ("one", 3))):
        text = fr.span_bytes_host(files["mixed"], "chrA")
        lines = fx.split_lines(text)
        allow_set = set() if allow == "-" else fx.parse_allowlist(bytes(ARRAYS[f"allow_{allow}"]))
        assert host(counts[k]).tobytes() == fx.count_region(lines, allow_set, 0, 100000, 50, 2000, mode, 0).tobytes()


# ---- 2. the structural edges, at sizes taken from the shape ----------------------------------------------------------------

def on_device(gpu, data: bytes, tail: int = 64):
    """The bytes on the device with a poisoned tail behind them that no kernel may read as text (it is all line feeds)."""
    import torch

    whole = torch.from_numpy(np.frombuffer(data + b"\n" * tail, dtype=np.uint8).copy()).to(gpu)
    return whole, whole[: len(data)]


def lines_of(gpu, data: bytes, entry0: int = 0):
    """`rocco_hip_fragfile_lines` with a guard element behind the n + 1 starts."""
    import torch

    from rocco_amd import _native, dp

    whole, view = on_device(gpu, data)
    lib, solver, back = _native.load(), _native.solver_for(gpu.index).handle, (ctypes.c_longlong * 4)()
    _native.check(lib.rocco_hip_fragfile_lines(solver, view.data_ptr(), len(data), entry0, None, 0, back, dp._stream_ptr(view)), "lines")
    n = int(back[0])
    starts = torch.full((n + 2,), POISON, dtype=torch.int64, device=gpu)
    _native.check(lib.rocco_hip_fragfile_lines(solver, view.data_ptr(), len(data), entry0, starts.data_ptr(), n + 1, back, dp._stream_ptr(view)), "lines")
    assert int(starts[n + 1]) == POISON
    if n > 0:
        assert lib.rocco_hip_fragfile_lines(solver, view.data_ptr(), len(data), entry0, starts.data_ptr(), n, back, dp._stream_ptr(view)) == _native.EINVAL
    return view, starts[: n + 1], (n, int(back[1]), bool(back[2]))


def test_the_line_pass_at_its_tile_edges(gpu):
    shape = fr.fragfile_shape()
    tile, lane = shape["tile_bytes"], shape["tile_bytes"] // shape["threads"]
    cases = [b"", b"\n", b"a", b"a\n", b"\n\n\n", b"abc\ndef", b"x" * (tile - 1) + b"\n",            # '\n' as the last byte of a tile
             b"x" * (tile - 1) + b"\n" + b"y" * 5, b"x" * tile + b"\ny\n",                          # ... and as the first of the next
             b"ab\n" + b"x" * (2 * tile + 100) + b"\ncd\n",                                         # a line that spans three tiles
             b"x" * (lane - 1) + b"\n" + b"y" * lane + b"\n" + b"\n" * (3 * lane) + b"z" * (tile + 3),
             b"".join(b"%d\n" % i for i in range(3000))]
    for data in cases:
        for entry0 in sorted({0, min(3, len(data)), min(tile, len(data)), min(tile + 1, len(data)), len(data)}):
            twin = fr.fragfile_host(data, entry0=entry0, fields=False)
            _, starts, report = lines_of(gpu, data, entry0)
            assert report == (twin["lines"], twin["cut"], twin["open"]), (len(data), entry0)
            assert np.array_equal(host(starts), twin["starts"]), (len(data), entry0)


def synthetic_text(n_lines: int, seed: int):
    """n_lines sound lines of one contig, starts ascending, fields of changing widths, a meta line now and then."""
    rng = np.random.default_rng(seed)
    starts = np.cumsum(rng.integers(0, 4, size=n_lines)) + 5
    widths = rng.integers(1, 700, size=n_lines)
    weights = rng.integers(0, 4, size=n_lines)
    barcodes = [b"AAAC", b"AAAG", b"CCGT", b"", b"TTTTTTTTTTTT"]
    picks = rng.integers(0, len(barcodes), size=n_lines)
    out = []
    for i in range(n_lines):
        if i % 9973 == 5000:
            out.append(b"#meta\n")
        out.append(b"c\t%d\t%d\t%s\t%d\n" % (starts[i], starts[i] + widths[i], barcodes[picks[i]], weights[i]))
    return b"".join(out)


def test_second_turns_of_the_line_field_count_range_and_mapped_kernels(gpu):
    """One byte more than cap x tile bytes and one line more than cap x lines-per-turn (the field kernels' cap, which is the
    larger): every kernel's workgroups take a second turn; GPU against the host twin and the integer statement."""
    shape = fr.fragfile_shape()
    n_lines = max(shape["fields_max_grid"], shape["count_max_grid"]) * shape["lines_per_turn"] + 1
    data = synthetic_text(n_lines, 7)
    assert len(data) > shape["lines_max_grid"] * shape["tile_bytes"] + 1
    allow = fr.parse_barcode_allowlist(b"AAAC\nCCGT\nTTTTTTTTTTTT\nAAA\n")
    twin = fr.fragfile_host(data, names=["c"], expect=[0], allowlists=[allow])
    assert twin["report"] == (-1, 0) and twin["lines"] > n_lines
    view, starts, report = lines_of(gpu, data)
    assert report == (twin["lines"], len(data), False) and np.array_equal(host(starts), twin["starts"])
    lines, found = fr.fields_device(view, starts, False, [0, twin["lines"]], [0], ["c"], [allow])
    assert found == (-1, 0)
    assert_lines_equal(lines, twin, "synthetic")
    top = int(twin["end"].max()) + 1
    for mode, one, region in ((0, 0, (0, top, 50)), (1, 0, (1000, top - 1000, 7)), (3, 0, (0, top, 1000)), (0, 1, (33, top // 2, 50))):
        (got,), (magnitude,) = fr.count_lines_batch_device([lines], [region], [mode], [one])
        length = ((region[1] - region[0] - 1) // region[2]) + 1
        want, want_magnitude = fx.counts_from_fields(twin["start"], twin["end"], twin["weight"], twin["status"], *region, length, mode, one)
        assert host(got).tobytes() == want.tobytes() and magnitude == want_magnitude, (mode, one)
    valid = ((twin["status"] & (fr.START_OK | fr.END_OK)) == (fr.START_OK | fr.END_OK)) & (twin["end"] > twin["start"])
    first, last = np.flatnonzero(valid)[0], np.flatnonzero(valid & (twin["start"] < 20000))[-1]
    assert fr.chrom_ranges_batch_device([lines], [20000]) == [(int(twin["start"][first]), int(twin["end"][last]))]
    whole = fr.fragfile_host(data, whole_file=True, names=["x"], allowlists=[allow])
    lines_w, found = fr.fields_device(view, starts, True, [0, twin["lines"]], [-1], ["x"], [allow])
    assert found == (-1, 0)
    assert_lines_equal(lines_w, whole, "synthetic, whole file")
    ok = (whole["name"] < 0) & ((whole["status"] & fr.FIFTH_EMPTY) == 0) & ((whole["status"] & fr.BARCODE_ALLOWED) != 0)
    assert fr.mapped_count_device(lines_w, 1, 0) == 2 * int(whole["weight"][ok].astype(np.int64).sum())
    assert fr.mapped_count_device(lines_w, 1, 1) == int(whole["weight"][ok].astype(np.int64).sum())


def test_zero_lines_one_line_and_guarded_outputs(gpu):
    import torch

    for data in (b"", b"c\t5\t9", b"c\t5\t9\n", b"#only\n"):
        view, starts, report = lines_of(gpu, data)
        twin = fr.fragfile_host(data, names=["c"], expect=[0])
        lines, found = fr.fields_device(view, starts, False, [0, report[0]], [0], ["c"], [fr._NO_LIST])
        assert found == twin["report"] == (-1, 0) and len(lines) == twin["lines"]
        assert_lines_equal(lines, twin, data)
        (got,), (magnitude,) = fr.count_lines_batch_device([lines], [(0, 100, 10)], [0], [0])
        assert host(got).tolist() == ([1.0 if data[:1] == b"c" else 0.0] + [0.0] * 9) and magnitude == (1 if data[:1] == b"c" else 0)
        assert fr.chrom_ranges_batch_device([lines], [100]) == [(5, 9) if data[:1] == b"c" else (0, 0)]
        assert fr.mapped_count_device(lines, 0, 0) == 0
    # the count writes its n_bins and nothing behind them: the buffer is fresh, its tail keeps what the caller put there
    from rocco_amd import _native, dp, readtracks as rt

    view, starts, report = lines_of(gpu, b"c\t5\t95\tB\t3\nc\t40\t41\n")
    lines, _ = fr.fields_device(view, starts, False, [0, 2], [0], ["c"], [fr._NO_LIST])
    out = torch.full((16,), float("nan"), dtype=torch.float32, device=gpu)
    regs, opts = (rt.CountRegion * 1)(rt.CountRegion(0, 100, 10, 10)), (fr._ModeOptions * 1)(fr._ModeOptions(0, 0))
    maxima = (ctypes.c_longlong * 1)()
    _native.check(_native.load().rocco_hip_fragfile_count_batch(
        _native.solver_for(gpu.index).handle, lines.start.data_ptr(), lines.end.data_ptr(), lines.weight.data_ptr(), lines.status.data_ptr(),
        fr._ll_p(fr._ll([0, 2])), 1, ctypes.cast(opts, ctypes.c_void_p), ctypes.cast(regs, ctypes.c_void_p), fr._ll_p(fr._ll([3])), out.data_ptr(),
        maxima, dp._stream_ptr(out)), "count")
    got = host(out)
    assert np.isnan(got[:3]).all() and np.isnan(got[13:]).all() and got[3:13].tolist() == [3, 3, 3, 3, 4, 3, 3, 3, 3, 3] and maxima[0] == 4


def test_the_field_report_names_the_first_offending_line_and_its_lowest_code(gpu):
    shape = fr.fragfile_shape()
    sound = [b"c\t%d\t%d\n" % (i, i + 3) for i in range(2 * shape["threads"] + 7)]
    for at, line, code in ((0, b"c\t01\t5\n", fr.ERR_NONCANONICAL), (shape["threads"], b"d\t300\t301\n", fr.ERR_CONTIG),
                           (2 * shape["threads"] + 6, b"c\t5\t9\n", fr.ERR_ORDER), (shape["threads"] - 1, b"c\t255\n", fr.ERR_FIELDS)):
        body = list(sound)
        body[at] = line
        body[-1] = body[-1] if at == len(body) - 1 else b"c\tx\t1\x00\n"  # (a later, worse line must not win)
        data = b"".join(body)
        view, starts, report = lines_of(gpu, data)
        _, found = fr.fields_device(view, starts, False, [0, report[0]], [0], ["c"], [fr._NO_LIST])
        assert found == (at, code) == fr.fragfile_host(data, names=["c"], expect=[0])["report"]


def test_all_lines_in_one_bin_reach_exactly_two_to_the_24_and_one_more(gpu):
    """A weight pile: 2**24 is accepted (float32 holds it), 2**24 + 1 is refused -- in P for the cut modes and the centre, in
    the running value for coverage."""
    n = 4096
    each = (1 << 24) // n
    text = b"".join(b"c\t500\t510\tB\t%d\n" % each for _ in range(n))
    view, starts, report = lines_of(gpu, text)
    lines, found = fr.fields_device(view, starts, False, [0, n], [0], ["c"], [fr._NO_LIST])
    assert found == (-1, 0)
    for mode in (0, 3):
        (got,), (magnitude,) = fr.count_lines_batch_device([lines], [(0, 1000, 100)], [mode], [0])
        assert magnitude == 1 << 24 and host(got)[5] == float(1 << 24) and host(got).sum() == float(1 << 24)
    view, starts, report = lines_of(gpu, text + b"c\t505\t506\n")
    more, _ = fr.fields_device(view, starts, False, [0, n + 1], [0], ["c"], [fr._NO_LIST])
    for mode in (0, 1, 3):
        with pytest.raises(RuntimeError, match=r"of track 0 reach \d+, beyond 2\*\*24"):
            fr.count_lines_batch_device([more], [(0, 1000, 100)], [mode], [0])
    _, maxima = fr.count_lines_batch_device([more, lines], [(0, 1000, 100)] * 2, [1, 1], [0, 1], check=False)
    assert maxima == [2 * (1 << 24) + 2, 1 << 24]  # (both cuts of every line fall into the one bin; the centre of the pile alone)


def test_one_track_and_seventy_tracks(gpu):
    rng = np.random.default_rng(11)
    texts, twins = [], []
    for k in range(70):
        n = int(rng.integers(0, 40)) if k % 7 else 0
        s = np.sort(rng.integers(0, 5000, size=n))
        texts.append(b"".join(b"c%d\t%d\t%d\tB\t%d\n" % (k, a, a + rng.integers(1, 400), rng.integers(1, 4)) for a in s))
    data = b"".join(texts)
    view, starts, report = lines_of(gpu, data)
    track_first = np.concatenate([[0], np.cumsum([t.count(b"\n") for t in texts])])
    names = [f"c{k}" for k in range(70)]
    lines, found = fr.fields_device(view, starts, False, track_first, list(range(70)), names, [fr._NO_LIST] * 70)
    assert found == (-1, 0)
    tracks = [lines.slice(int(track_first[k]), int(track_first[k + 1])) for k in range(70)]
    regions = [(10 * k, 5000 + k, 1 + k % 13) for k in range(70)]
    modes, ones = [k % 4 for k in range(70)], [(k // 4) % 2 for k in range(70)]
    counts, maxima = fr.count_lines_batch_device(tracks, regions, modes, ones)
    ranges = fr.chrom_ranges_batch_device(tracks, [4000 + 10 * k for k in range(70)])
    for k in range(70):
        twin = fr.fragfile_host(texts[k], names=[names[k]], expect=[0])
        length = ((regions[k][1] - regions[k][0] - 1) // regions[k][2]) + 1
        want, magnitude = fx.counts_from_fields(twin["start"], twin["end"], twin["weight"], twin["status"], *regions[k], length, modes[k], ones[k])
        assert host(counts[k]).tobytes() == want.tobytes() and maxima[k] == magnitude, k
        kept = [line for line in fx.split_lines(texts[k]) if int(line.split(b"\t")[1]) < 4000 + 10 * k]
        assert ranges[k] == fx.chrom_range(kept), k
    (alone,), _ = fr.count_lines_batch_device([tracks[3]], [regions[3]], [modes[3]], [ones[3]])
    assert host(alone).tobytes() == host(counts[3]).tobytes()


def test_a_line_outside_the_dialect_is_a_value_error_that_names_it(gpu, files, tmp_path):
    """A file whose index is another file's: the span does not hold the contig's lines."""
    import shutil

    other = str(tmp_path / "other.tsv.gz")
    shutil.copy(files["plain"], other)
    shutil.copy(files["blocks"] + ".tbi", other + ".tbi")
    with pytest.raises(ValueError) as caught:
        fr.read_fragments_spans([(other, "chrB")], device=gpu)
    assert other in str(caught.value) and "contig chrB" in str(caught.value)


# ---- 3. the path functions -------------------------------------------------------------------------------------------------

def test_chrom_reads_metadata_matrix_and_run_chromosomes(gpu, files, tmp_path, monkeypatch):
    """`get_fragments_chrom_reads` from its parts (the stored range, the window the reference derives, the stored counts of that
    window, the reference's tail in NumPy); `generate_chrom_matrix` against it and the assembly by hand; `run_chromosomes` from
    fragments sources against the same matrices handed in directly, BED bytes equal."""
    from rocco_amd import readtracks as rt
    from rocco_amd import rocco as impl

    fr.clear_fragments_cache()
    sources = [source(files, "plain"), source(files, "plain", "many"), source(files, "mixed", "many"), source(files, "blocks")]
    step, sizes = 50, META["sizes"]
    metadata = fr._get_fragments_count_metadata(sources[0], step, "RPKM", -1, ["chrX"])
    mapped = next(r for r in META["mapped"] if r["file"] == "plain" and r["mode"] == "coverage" and r["allow"] == "-" and not r["exclude"])
    length = next(r for r in META["readlen"] if r["file"] == "plain" and r["min_reads"] == 32)
    assert metadata["mapped_reads"] == mapped["mapped"] and metadata["read_length"] == length["read_length"] and metadata["paired_end"] is False
    assert metadata["norm_scale"] == rt._compute_native_scale_factor("RPKM", -1, step, mapped["mapped"], length["read_length"], 1.0)
    with pytest.raises(RuntimeError, match="source kind is not BAM"):
        fr._get_fragments_count_metadata(sources[0], step, "RPKM", -1, None, extend_reads=0)
    stored = next(r for r in META["count"] if r["name"] == "window_plain_chrA_50")
    intervals, vals = fr.get_fragments_chrom_reads(sources[0], "chrA", files["sizes"], step, norm_method="RPKM", ignore_for_norm=["chrX"])
    want = ARRAYS["c_window_plain_chrA_50"].astype(np.float64) * metadata["norm_scale"] * 1.0
    support = np.flatnonzero(want > 0.0)
    assert np.array_equal(intervals, stored["start"] + step * np.arange(support[0], support[-1] + 1))
    assert np.array_equal(vals, np.round(want[support[0]: support[-1] + 1], 5)) and intervals.dtype == int
    assert fr.get_fragments_chrom_reads(sources[0], "chrB", files["sizes"], step, norm_method="CPM") == (None, None)
    with pytest.raises(ValueError, match="Chromosome chrD not found in chromosome sizes file"):
        fr.get_fragments_chrom_reads(sources[2], "chrD", files["sizes"], step)
    with pytest.raises(FileNotFoundError, match="BAM file not found"):
        fr.get_fragments_chrom_reads(str(tmp_path / "none.tsv.gz"), "chrA", files["sizes"], step)

    kwargs = dict(norm_method="CPM", count_mode="cutsite")
    by_hand = [fr.get_fragments_chrom_reads(s, "chrA", files["sizes"], step, **kwargs) for s in sources]
    want_starts, want_matrix = rt.assemble_chrom_matrix([i for i, _ in by_hand], [v for _, v in by_hand], track_type="bam")
    before = fr._LoadCounts.inflates
    starts, matrix = fr.generate_chrom_matrix("chrA", sources, files["sizes"], step, **kwargs)
    assert fr._LoadCounts.inflates == before and np.array_equal(starts, want_starts) and matrix.tobytes() == want_matrix.tobytes()
    assert matrix.shape[0] == 4 and not np.array_equal(matrix[0], matrix[1])
    assert fr.generate_chrom_matrix("chrB", sources[:2], files["sizes"], step, norm_method="CPM") == (None, None)

    chroms = ["chrA", "chrE"]
    args = {"chrom_sizes_file": files["sizes"], "step": step, "round_digits": 5, "effective_genome_size": -1, "norm_method": "CPM",
            "min_mapping_score": 10, "flag_include": None, "flag_exclude": 3844, "extend_reads": -1, "center_reads": False,
            "ignore_for_norm": None, "scale_factor": 1.0, "score_lower_bound_z": 1.0, "score_prior_df": 6.0, "score_min_effect": None,
            "score_precision_floor_ratio": 0.01, "gamma": None, "budget": None, "scale_chrom_budgets": 1.0, "budget_posterior_quantile": 0.01,
            "selection_penalty": None, "min_length_bp": 100, "narrowPeak": False, "low_memory": False, "input_track_type": "bam",
            "budget_null_draws": 6, "threads": 1}
    three = [source(files, "plain"), source(files, "plain", "many"), source(files, "mixed", "many")]
    from_matrices = {c: fr.generate_chrom_matrix(c, three, files["sizes"], step, norm_method="CPM") for c in chroms}
    monkeypatch.chdir(tmp_path)
    want_bed = impl.run_chromosomes(chroms, from_matrices, dict(args, output=str(tmp_path / "want.bed")), run_id="1")
    monkeypatch.setattr(impl, "generate_chrom_matrix", fr.generate_chrom_matrix_device)
    got_bed = impl.run_chromosomes(chroms, three, dict(args, output=str(tmp_path / "got.bed")), run_id="2")
    with open(want_bed, "rb") as a, open(got_bed, "rb") as b:
        want_bytes, got_bytes = a.read(), b.read()
    assert len(want_bytes) > 0 and got_bytes == want_bytes


# ---- 4. the Python level against the reference's own readtracks.py --------------------------------------------------------

TAIL_DEFAULTS = dict(effective_genome_size=2.7e9, norm_method="RPGC", min_mapping_score=10, flag_include=None, flag_exclude=3844, extend_reads=-1,
                     center_reads=False, ignore_for_norm=None, scale_factor=1.0, num_processors=1, const_scale=1.0, round_digits=5,
                     scale_by_step=False)


def log_of(caplog, path):
    return [[r.levelname, r.getMessage().replace(path, "{file}")] for r in caplog.records if r.name == fr.logger.name]


@pytest.mark.parametrize("scenario", META["tail"], ids=[t["name"] for t in META["tail"]])
def test_the_path_functions_against_the_references_own_python(gpu, files, caplog, scenario):
    """What the reference's `get_bam_chrom_reads` and `_get_bam_count_metadata` returned, logged and raised over a stand-in that
    forwards to its compiled counter with the fragments source kind (tests/golden/make_golden_fragments.py step 3):
    (intervals, values) bit for bit, the metadata dict, every log record at INFO and above in order, the (None, None) cases
    with their warnings, the exception types and words."""
    import logging

    fr.clear_fragments_cache()
    src = source(files, scenario["file"], scenario["allow"])
    call = dict(TAIL_DEFAULTS, **scenario["kwargs"])
    caplog.set_level(logging.INFO, logger=fr.logger.name)
    caplog.clear()
    if "exception" in scenario:
        kind, words = scenario["exception"]
        with pytest.raises({"RuntimeError": RuntimeError, "ValueError": ValueError}[kind]) as caught:
            fr.get_fragments_chrom_reads(src, scenario["contig"], files["sizes"], scenario["step"], count_mode=scenario["mode"], **call)
        assert type(caught.value).__name__ == kind
        assert words.replace("{file}", src.path).replace("{sizes}", files["sizes"]) in str(caught.value)
        assert log_of(caplog, src.path) == scenario["log"]
        return
    intervals, vals = fr.get_fragments_chrom_reads(src, scenario["contig"], files["sizes"], scenario["step"], count_mode=scenario["mode"], **call)
    assert log_of(caplog, src.path) == scenario["log"]
    metadata = fr._get_fragments_count_metadata(src, step=scenario["step"], norm_method=call["norm_method"],
                                                effective_genome_size=call["effective_genome_size"],
                                                ignore_for_norm=call["ignore_for_norm"] or ["chrX", "chrY", "chrM"], flag_exclude=call["flag_exclude"],
                                                extend_reads=call["extend_reads"], num_processors=1, scale_factor=call["scale_factor"])
    assert metadata == scenario["metadata"] and all(type(metadata[k]) is type(v) for k, v in scenario["metadata"].items())
    if scenario.get("none"):
        assert intervals is None and vals is None
    else:
        want_i, want_v = ARRAYS[f"t_{scenario['name']}_intervals"], ARRAYS[f"t_{scenario['name']}_values"]
        assert str(intervals.dtype) == scenario["intervals_dtype"] and str(vals.dtype) == scenario["values_dtype"]
        assert np.array_equal(intervals, want_i) and vals.tobytes() == want_v.tobytes()


def test_the_tail_scenarios_cover_what_the_issue_names():
    tail = META["tail"]
    assert {t["mode"] for t in tail if "metadata" in t and not t.get("none")} == set(MODES)
    assert len({t["step"] for t in tail}) >= 4 and any(t["kwargs"].get("center_reads") for t in tail)
    warned = [t["log"][-1][1] for t in tail if t.get("none")]
    assert any("No mapped reads found" in w for w in warned) and any("No non-zero values found" in w for w in warned)
    assert sum("No mapped reads found" in w for w in warned) >= 2  # (a contig the index does not know, a contig without a valid line)
    assert ["RuntimeError", "source kind is not BAM"] in [t.get("exception") for t in tail]


def test_the_matrix_logs_file_by_file_as_the_reference_does(gpu, files, caplog):
    """`generate_chrom_matrix` over K sources: the records of source 0, then those of source 1, ... (the reference calls
    `get_bam_chrom_reads` file by file), then one exclusion warning per source without data."""
    import logging

    sources = [source(files, "plain"), source(files, "novalid"), source(files, "plain", "absent"), source(files, "plain", "many")]
    kwargs = dict(norm_method="CPM", scale_by_step=True)
    caplog.set_level(logging.INFO, logger=fr.logger.name)
    want = []
    for src in sources:
        caplog.clear()
        fr.get_fragments_chrom_reads(src, "chrA", files["sizes"], 50, num_processors=1, **kwargs)
        want += [[r.levelname, r.getMessage()] for r in caplog.records if r.name == fr.logger.name]
    want.append(["WARNING", f"No data found for {sources[2].path} in chromosome chrA. Excluding this track for chrA."])
    caplog.clear()
    starts, matrix = fr.generate_chrom_matrix("chrA", sources, files["sizes"], 50, num_processors=1, **kwargs)
    assert [[r.levelname, r.getMessage()] for r in caplog.records if r.name == fr.logger.name] == want
    assert matrix.shape[0] == 3 and [w[1][:8] for w in want].count("Dividing") == 4 and sum("No non-zero" in w[1] for w in want) == 1


# ---- 5. empty streams in a group, guards behind the field outputs ----------------------------------------------------------

def test_a_known_contig_without_lines_among_the_sources_of_a_group(gpu, files, tmp_path):
    """A contig the index names but has no bin for (an empty stream) between two sources with lines: empty lines for it, a
    range of 0 / 0, zero counts, over zero-length tensors."""
    import shutil

    from rocco_amd import bam_index

    real = tabix_index.open_tabix_index(files["plain"])
    path = str(tmp_path / "hollow.tsv.gz")
    shutil.copy(files["plain"], path)
    fx.write_tbi(path + ".tbi", [("chrA", bam_index.contig_span(real, 0)), ("chrZ", None), ("chrE", bam_index.contig_span(real, 1))])
    fr.clear_fragments_cache()
    before = fr._LoadCounts.inflates
    got = fr.read_fragments_spans([(path, "chrA"), (path, "chrZ"), (files["blocks"], "chrA"), (path, "chrZ"), (path, "chrNone")], device=gpu)
    assert fr._LoadCounts.inflates == before + 1 and got[4] is None and len(got[1]) == len(got[3]) == 0 and len(got[0]) > 0
    twin = fr.fragfile_host(fr.span_bytes_host(files["plain"], "chrA"), names=["chrA"], expect=[0])
    assert_lines_equal(got[0], twin, "hollow chrA", name_index=None)
    assert fr.span_bytes_host(path, "chrZ") == b""
    counts, maxima = fr.count_lines_batch_device([got[1], got[0], got[3]], [(0, 1000, 10), (0, 200000, 50), (5, 77, 1)], [0, 1, 3], [0, 0, 1])
    assert not host(counts[0]).any() and not host(counts[2]).any() and host(counts[1]).any() and maxima[0] == maxima[2] == 0
    assert fr.chrom_ranges_batch_device([got[1], got[0], got[3]], [1000, 200000, 1000])[::2] == [(0, 0), (0, 0)]
    (alone,), (zero,) = fr.count_lines_batch_device([got[1]], [(0, 1000, 10)], [0], [0])
    assert alone.shape[0] == 100 and not host(alone).any() and zero == 0 and fr.chrom_ranges_batch_device([got[1]], [1000]) == [(0, 0)]
    assert fr.get_fragments_chrom_range(path, "chrZ", 1000) == (0, 0) and not fr.count_fragments_region(path, "chrZ", 0, 500, 50).any()


def test_guard_elements_behind_the_five_field_outputs(gpu):
    import torch

    from rocco_amd import _native, dp

    shape = fr.fragfile_shape()
    data = b"".join(b"c\t%d\t%d\tAB\t%d\n" % (i, i + 9, 1 + i % 3) for i in range(shape["threads"] + 3))
    view, starts, report = lines_of(gpu, data)
    n = report[0]
    outs = [torch.full((n + 2,), POISON & 0x7FFFFFFF, dtype=torch.int32, device=gpu) for _ in range(5)]
    name_bytes, name_offsets = fr._names_table(["c"])
    allow_first, allow_offsets, allow_bytes, entries = fr._pack_allowlists([fr.parse_barcode_allowlist(b"AB\n")])
    allow_bytes_t, allow_offsets_t = torch.from_numpy(allow_bytes).to(gpu), torch.from_numpy(allow_offsets).to(gpu)
    back, first, expect = (ctypes.c_longlong * 4)(), fr._ll([0, n]), np.zeros(1, dtype=np.int32)
    allow_first_a = fr._ll(allow_first)
    _native.check(_native.load().rocco_hip_fragfile_fields(
        _native.solver_for(gpu.index).handle, view.data_ptr(), len(data), starts.data_ptr(), n, 0, fr._ll_p(first),
        expect.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1, name_bytes.ctypes.data, fr._ll_p(name_offsets), 1, allow_bytes_t.data_ptr(),
        allow_offsets_t.data_ptr(), entries, fr._ll_p(allow_first_a), *[o[1:].data_ptr() for o in outs], back, dp._stream_ptr(view)), "fields")
    twin = fr.fragfile_host(data, names=["c"], expect=[0], allowlists=[fr.parse_barcode_allowlist(b"AB\n")])
    assert (int(back[0]), int(back[1])) == (-1, 0)
    for out, name in zip(outs, ("start", "end", "weight", "name", "status")):
        got = host(out)
        assert got[0] == got[-1] == POISON & 0x7FFFFFFF, name
        assert np.array_equal(got[1:-1].view(twin[name].dtype), twin[name]), name
