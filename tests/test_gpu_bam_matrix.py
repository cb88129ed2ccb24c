"""GPU: K BAM files of one chromosome to the reference's (common_intervals, count_matrix) in one device pass (DESIGN.md
section 0 row f9).

1. rocco_amd.bam.generate_chrom_matrix / generate_chrom_matrix_device against what the REFERENCE's own generate_chrom_matrix
   returned (tests/golden/bam_files.npz and bam_matrix.npz): intervals, the matrix by its bit pattern and dtype, the
   (None, None) returns, the errors, and every WARNING / INFO record of the call in order.
2. rocco_amd.readtracks.bam_chrom_matrix_from_records_batch against the existing route (bam_chrom_reads_from_records_batch
   then assemble_chrom_matrix_device, itself pinned to the reference) on synthetic records the fixtures cannot reach.
3. The binding of INTEGRATION.md: run_chromosomes from BAM paths writes the bytes it writes from the fixture matrices."""
import logging

import numpy as np
import pytest

import bam_expected as bx
import bam_matrix_cases as mx

pytestmark = pytest.mark.gpu

NO_READS = "No mapped reads found in BAM file: {f} for chromosome: {c}. Returning (None,None)."
NO_VALUES = "No non-zero values found in BAM file: {f} for chromosome: {c}. Returning (None,None)."
EXCLUDED = "No data found for {f} in chromosome {c}. Excluding this track for {c}."
NOTHING = "No data found in the files {fs} for chromosome {c}. Returning (None,None)."
ZERO = "You are scaling the values by 0."


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    from rocco_amd import bam

    bam.clear_alignment_cache()
    yield mx.write_files(tmp_path_factory.mktemp("bam_matrix"))
    bam.clear_alignment_cache()


class Keep(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.DEBUG)
        self.records = []

    def emit(self, record):
        self.records.append([record.levelname, record.getMessage()])


def logged(call, paths=None, clear_metadata=True):
    """(result, the WARNING and INFO records of rocco_amd's reader during the call, file paths replaced by their keys)."""
    from rocco_amd import bam

    keep = Keep()
    bam.logger.addHandler(keep)
    level = bam.logger.level
    bam.logger.setLevel(logging.DEBUG)
    if clear_metadata:
        bam._BAM_COUNT_METADATA_CACHE.clear()
    try:
        result = call()
    finally:
        bam.logger.removeHandler(keep)
        bam.logger.setLevel(level)
        log = []
        for level_name, message in keep.records:
            for key, path in (paths or {}).items():
                message = message.replace(path, "{" + key + "}")
            if level_name in ("WARNING", "INFO"):
                log.append([level_name, message])
        logged.last = log
    return result, log


def same_bits(got, want) -> bool:
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


# ---- 1. the reference's fixtures -------------------------------------------------------------------------------------------
def _scenarios():
    _, old = bx.golden()
    _, new = mx.golden()
    return [("old", r["name"]) for r in old["matrix"]] + [("new", e["name"]) for e in new["scenarios"]]


@pytest.mark.parametrize("which,name", _scenarios())
def test_generate_chrom_matrix_as_the_reference_ran_it(gpu, paths, which, name):
    import torch

    from rocco_amd import bam

    if which == "old":
        arrays, meta = bx.golden()
        entry = dict(next(r for r in meta["matrix"] if r["name"] == name), error=None, none=False)
        want_i, want_m = arrays[f"{name}_intervals"], arrays[f"{name}_matrix"]
    else:
        arrays, meta = mx.golden()
        entry = next(e for e in meta["scenarios"] if e["name"] == name)
        want_i, want_m = arrays.get(f"{name}_intervals"), arrays.get(f"{name}_matrix")
    want_log = [r for r in entry["log"] if r[0] in ("WARNING", "INFO")]
    files = [paths[k] for k in entry["files"]]
    for function in (bam.generate_chrom_matrix, bam.generate_chrom_matrix_device):
        call = lambda: function(entry["contig"], files, paths["sizes"], entry["step"], **entry["kwargs"])
        if entry["error"] is not None:
            with pytest.raises({"RuntimeError": RuntimeError, "ValueError": ValueError}[entry["error_type"]]) as info:
                logged(call, paths)
            assert str(info.value).replace(paths["sizes"], "{sizes}") == entry["error"] and logged.last == want_log
            continue
        (intervals, matrix), log = logged(call, paths)
        assert log == want_log
        if entry["none"]:
            assert intervals is None and matrix is None
            continue
        assert isinstance(intervals, np.ndarray) and intervals.dtype == want_i.dtype and np.array_equal(intervals, want_i)
        if function is bam.generate_chrom_matrix_device:
            assert isinstance(matrix, torch.Tensor) and matrix.is_cuda
            matrix = matrix.cpu().numpy()
        assert isinstance(matrix, np.ndarray) and same_bits(matrix, want_m)
        assert same_bits(matrix.view(np.int32 if matrix.dtype == np.float32 else np.int64),
                         want_m.view(np.int32 if want_m.dtype == np.float32 else np.int64))


def test_reader_checks_come_first_and_are_the_references(gpu, paths, tmp_path):
    """The file type, the two FileNotFoundErrors and the chromosome ValueError, for the first offending file."""
    from rocco_amd import bam

    _, old = bx.golden()
    by_label = {e["label"]: e for e in old["errors"]}
    missing_bam, missing_sizes = str(tmp_path / "none.bam"), str(tmp_path / "none.sizes")
    with pytest.raises(FileNotFoundError) as info:
        bam.generate_chrom_matrix_device("chrA", [paths["mixed"], missing_bam], paths["sizes"], 50, norm_method="CPM")
    assert str(info.value).replace(missing_bam, "{bam}") == by_label["missing_bam"]["message"]
    with pytest.raises(FileNotFoundError) as info:
        bam.generate_chrom_matrix("chrA", [paths["mixed"]], missing_sizes, 50)
    assert str(info.value).replace(missing_sizes, "{sizes}") == by_label["missing_sizes"]["message"]
    with pytest.raises(ValueError) as info:
        bam.generate_chrom_matrix("chrQ", [paths["mixed"]], paths["sizes"], 50)
    assert str(info.value).replace(paths["sizes"], "{sizes}") == by_label["missing_chromosome"]["message"]
    with pytest.raises(ValueError, match="All input files must share the same type."):
        bam.generate_chrom_matrix("chrA", [paths["mixed"], "x.bw"], paths["sizes"], 50)
    with pytest.raises(ValueError, match=r"Unsupported input file type for `x\.txt`\. Expected BAM or bigWig\."):
        bam.generate_chrom_matrix("chrA", ["x.txt"], paths["sizes"], 50)
    with pytest.raises(ValueError, match="reads BAM files"):
        bam.generate_chrom_matrix_device("chrA", ["x.bw"], paths["sizes"], 50)


def test_metadata_comes_from_the_cache_the_second_time(gpu, paths):
    """The metadata lines belong to the first call with a key; the second call logs the counting's records only."""
    from rocco_amd import bam

    _, meta = mx.golden()
    entry = next(e for e in meta["scenarios"] if e["name"] == "scale_by_step")
    call = lambda: bam.generate_chrom_matrix_device(entry["contig"], [paths[k] for k in entry["files"]], paths["sizes"], entry["step"],
                                                     **entry["kwargs"])
    (_, first), _ = logged(call, paths)
    (_, second), log = logged(call, paths, clear_metadata=False)
    assert log == [["INFO", "Dividing `vals` by step size (bp): 200"]] * len(entry["files"])
    assert same_bits(first.cpu().numpy(), second.cpu().numpy())


# ---- 2. against the existing route ------------------------------------------------------------------------------------------
def old_route(records_list, chrom_size, step, metas, low_memory=False, **kw):
    from rocco_amd import readtracks as rt

    intervals, vals = rt.bam_chrom_reads_from_records_batch(records_list, chrom_size, step, metas, **kw)
    kept = [(i, v) for i, v in zip(intervals, vals) if i is not None]
    if not kept:
        return None, None
    common, matrix = rt.assemble_chrom_matrix_device([i for i, _ in kept], [v for _, v in kept], low_memory=low_memory)
    return common.cpu().numpy().astype(int), matrix


def both_routes(tracks, chrom_size, step=mx.STEP, scales=None, names=None, **kw):
    """(starts, matrix, log) of the new call; asserts that the existing route gives the same starts and the same bits."""
    import torch

    from rocco_amd import readtracks as rt

    records = [rt.AlignmentRecords(*t) for t in tracks]
    metas = [mx.metadata(1.0 if scales is None else scales[k]) for k in range(len(tracks))]
    names = names if names is not None else [f"f{k}.bam" for k in range(len(tracks))]
    (starts, matrix), log = logged(lambda: rt.bam_chrom_matrix_from_records_batch(records, chrom_size, step, metas, bam_files=names,
                                                                                  chromosome="chrS", **kw))
    want_starts, want_matrix = old_route(records, chrom_size, step, metas, **kw)
    if want_starts is None:
        assert starts is None and matrix is None
        return starts, matrix, log
    assert isinstance(starts, np.ndarray) and starts.dtype == want_starts.dtype and np.array_equal(starts, want_starts)
    assert matrix.is_cuda and matrix.dtype == want_matrix.dtype and matrix.shape == want_matrix.shape
    bits = torch.int32 if matrix.dtype == torch.float32 else torch.int64
    assert torch.equal(matrix.view(bits), want_matrix.view(bits))
    return starts, matrix, log


def test_past_one_launchs_first_turn(gpu):
    """K' x m just past cap x unit: the last row's later columns are written by workgroups in their second turn.  Reads lie
    all along every row, so a turn left out, or taken twice at the wrong place, leaves other bits there."""
    from rocco_amd import readtracks as rt

    m = mx.second_turn_columns(rt.track_matrix_shape())
    tracks = [mx.bin_reads(mx.sparse_bins(0, m - 1, 5, keep=0.05), 6, depth=2),
              mx.bin_reads(mx.sparse_bins(777, m - 4000, 7, keep=0.05), 8, depth=2),
              mx.bin_reads(mx.sparse_bins(3, m - 1, 9, keep=0.05), 10, depth=2)]
    starts, matrix, log = both_routes(tracks, m * mx.STEP + 123, scales=[1.0, 0.25, 3.0])
    assert matrix.shape == (3, m) and log == []
    turn = rt.track_matrix_shape()["unit"] * rt.track_matrix_shape()["max_grid"]
    # (about one column in twenty holds reads: some hundreds of the second turn's 3 m - cap x unit elements)
    assert int((matrix.reshape(-1)[turn:] != 0).sum()) > (3 * m - turn) // 40, "nothing to get wrong in the second turn"


@pytest.mark.parametrize("low_memory", [False, True])
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 7, 8, 9, 1023, 1025])
def test_row_lengths_around_the_vector_width(gpu, m, low_memory):
    """m = 1, the 16-byte word of either dtype +- 1, a thread's four columns +- 1, a unit +- 1: rows of an odd length start
    off a 16-byte boundary (float32: rows 1 .. 3 at 4, 8 and 12 bytes), so heads and tails are stored one by one."""
    first = 40
    tracks = [mx.bin_reads(np.arange(first, first + m), 11 + m),
              mx.bin_reads(mx.sparse_bins(first, first + m - 1, 12 + m), 13),
              mx.bin_reads(mx.sparse_bins(first + m // 2, first + m - 1, 14 + m), 15),
              mx.bin_reads([first + m - 1], 16)]
    starts, matrix, _ = both_routes(tracks, 400000, scales=[1.0, 0.5, 2.0, 7.0], low_memory=low_memory)
    assert matrix.shape == (4, m) and starts[0] == first * mx.STEP


@pytest.mark.parametrize("low_memory", [False, True])
def test_nested_identical_disjoint_touching_and_single_bin_supports(gpu, low_memory):
    a = mx.sparse_bins(100, 199, 21)
    tracks = [mx.bin_reads(a, 22), mx.bin_reads(mx.sparse_bins(120, 150, 23), 24), mx.bin_reads(a, 22),
              mx.bin_reads(mx.sparse_bins(400, 449, 25), 26), mx.bin_reads(mx.sparse_bins(450, 470, 27), 28),
              mx.bin_reads([903], 29), mx.bin_reads(mx.sparse_bins(60, 99, 30), 31)]
    starts, matrix, log = both_routes(tracks, 60000, scales=[1.0, 2.0, 1.0, 0.1, 3.0, 1.5, 1.0], low_memory=low_memory)
    want = np.concatenate([np.arange(60, 200), np.arange(400, 471), [903]]) * mx.STEP
    assert np.array_equal(starts, want) and np.unique(np.diff(starts)).size == 3 and matrix.shape == (7, want.size) and log == []
    row = matrix[5].cpu().numpy()
    assert np.count_nonzero(row) == 1 and row[-1] > 0 and not np.signbit(row).any()


def test_tracks_without_data_are_dropped_with_the_references_records(gpu):
    """A track whose every read fails min_mapping_score has a range and no value; an empty track has no range."""
    tracks = [mx.bin_reads(mx.sparse_bins(10, 90, 41), 42), mx.bin_reads(mx.sparse_bins(20, 70, 43), 44, mapq=5), mx.empty_records(),
              mx.bin_reads(mx.sparse_bins(200, 260, 45), 46)]
    names = ["a.bam", "lowq.bam", "empty.bam", "d.bam"]
    starts, matrix, log = both_routes(tracks, 30000, names=names, scale_by_step=True)
    assert matrix.shape[0] == 2
    divide = ["INFO", f"Dividing `vals` by step size (bp): {mx.STEP}"]
    assert log == [divide, divide, ["WARNING", NO_VALUES.format(f="lowq.bam", c="chrS")], ["WARNING", NO_READS.format(f="empty.bam", c="chrS")],
                   divide, ["WARNING", EXCLUDED.format(f="lowq.bam", c="chrS")], ["WARNING", EXCLUDED.format(f="empty.bam", c="chrS")]]


def test_a_scale_of_zero_drops_everything(gpu):
    """const_scale = 0 (below the signature of generate_chrom_matrix): a positive count alone does not make a support."""
    tracks = [mx.bin_reads(mx.sparse_bins(10, 90, 51), 52), mx.bin_reads(mx.sparse_bins(20, 70, 53), 54)]
    names = ["a.bam", "b.bam"]
    starts, matrix, log = both_routes(tracks, 30000, names=names, const_scale=0)
    assert starts is None and matrix is None
    per_file = lambda f: [["WARNING", ZERO], ["WARNING", NO_VALUES.format(f=f, c="chrS")]]
    assert log == per_file("a.bam") + per_file("b.bam") + [["WARNING", EXCLUDED.format(f=f, c="chrS")] for f in names] + \
        [["WARNING", NOTHING.format(fs=str(names), c="chrS")]]
    # a zero or negative norm_scale, or one that underflows, of one file only
    starts, matrix, log = both_routes(tracks + [mx.bin_reads([33], 55), mx.bin_reads([34], 56)], 30000, scales=[0.0, 1.0, -2.0, 1e-320],
                                      names=["z.bam", "b.bam", "n.bam", "u.bam"], const_scale=1e-10)
    assert matrix.shape[0] == 1 and [r[1] for r in log if "Excluding" in r[1]] == [EXCLUDED.format(f=f, c="chrS") for f in ("z.bam", "n.bam", "u.bam")]
    # a negative const_scale is not applied (rocco/readtracks.py:500)
    starts, matrix, log = both_routes(tracks, 30000, const_scale=-3.0)
    assert matrix.shape[0] == 2 and float(matrix.min()) >= 0.0


def test_more_tracks_than_a_wavefront_has_lanes(gpu):
    rng = np.random.default_rng(61)
    tracks = []
    for k in range(70):
        first = int(rng.integers(0, 3000))
        tracks.append(mx.bin_reads(mx.sparse_bins(first, first + int(rng.integers(0, 900)), 62 + k), 200 + k))
    starts, matrix, _ = both_routes(tracks, 400000, scales=list(rng.uniform(0.1, 4.0, size=70)))
    assert matrix.shape[0] == 70
    starts, matrix, _ = both_routes(tracks, 400000, low_memory=True, round_digits=2, center_reads=True)
    assert matrix.shape[0] == 70


def test_only_the_last_track_has_data(gpu):
    tracks = [mx.empty_records() for _ in range(9)] + [mx.bin_reads(mx.sparse_bins(5, 3005, 71), 72)]
    starts, matrix, log = both_routes(tracks, 400000)
    assert matrix.shape == (1, 3001) and len(log) == 18
    assert log[:9] == [["WARNING", NO_READS.format(f=f"f{k}.bam", c="chrS")] for k in range(9)]
    # no file with records at all
    starts, matrix, log = both_routes([mx.empty_records(), mx.empty_records()], 400000)
    assert starts is None and log[-1] == ["WARNING", NOTHING.format(fs=str(["f0.bam", "f1.bam"]), c="chrS")]


def test_the_exact_count_guard_still_raises(gpu):
    """2**24 + 8 reads on one bin: float32 coverage is no longer exact, and there is no CPU fallback."""
    import torch

    from rocco_amd import readtracks as rt

    n = (1 << 24) + 8
    pile = rt.AlignmentRecords._of(torch.full((n,), 500, dtype=torch.int32, device=gpu), torch.full((n,), 550, dtype=torch.int32, device=gpu),
                                   torch.zeros(n, dtype=torch.int32, device=gpu), torch.zeros(n, dtype=torch.int16, device=gpu),
                                   torch.full((n,), 30, dtype=torch.uint8, device=gpu), torch.ones(n, dtype=torch.uint8, device=gpu))
    other = rt.AlignmentRecords(*mx.bin_reads(mx.sparse_bins(5, 50, 81), 82)).to(gpu)
    with pytest.raises(RuntimeError, match=r"alignment counts of track 1 reach \d+, beyond 2\*\*24"):
        rt.bam_chrom_matrix_from_records_batch([other, pile], 100000, mx.STEP, [mx.metadata(), mx.metadata()])


# ---- 3. the binding ------------------------------------------------------------------------------------------------------
def test_run_chromosomes_from_bam_paths_writes_the_same_bed(gpu, paths, tmp_path, monkeypatch):
    """rocco_amd.rocco.generate_chrom_matrix = rocco_amd.bam.generate_chrom_matrix_device: from three BAM
    paths to the combined BED, byte for byte what run_chromosomes writes from the reference's own matrices."""
    from rocco_amd import bam
    from rocco_amd import rocco as impl

    arrays, meta = mx.golden()
    entries = {e["contig"]: e for e in meta["scenarios"] if e["name"].startswith("all_")}
    chroms = ["chrA", "chrB", "chrC"]
    one = entries["chrA"]
    args = {"chrom_sizes_file": paths["sizes"], "step": one["step"], "round_digits": 5, "effective_genome_size": -1,
            "norm_method": one["kwargs"]["norm_method"], "min_mapping_score": 10, "flag_include": None, "flag_exclude": 3844,
            "extend_reads": -1, "center_reads": False, "ignore_for_norm": None, "scale_factor": 1.0, "score_lower_bound_z": 1.0,
            "score_prior_df": 6.0, "score_min_effect": None, "score_precision_floor_ratio": 0.01, "gamma": None, "budget": None,
            "scale_chrom_budgets": 1.0, "budget_posterior_quantile": 0.01, "selection_penalty": None, "min_length_bp": 100,
            "narrowPeak": False, "low_memory": False, "input_track_type": "bam", "budget_null_draws": 6,
            "threads": one["kwargs"]["num_processors"]}
    monkeypatch.chdir(tmp_path)
    from_matrices = {c: (arrays[f"all_{c}_intervals"], arrays[f"all_{c}_matrix"]) for c in chroms}
    want = impl.run_chromosomes(chroms, from_matrices, dict(args, output=str(tmp_path / "want.bed")), run_id="1")
    monkeypatch.setattr(impl, "generate_chrom_matrix", bam.generate_chrom_matrix_device)
    got = impl.run_chromosomes(chroms, [paths[k] for k in one["files"]], dict(args, output=str(tmp_path / "got.bed")), run_id="2")
    with open(want, "rb") as a, open(got, "rb") as b:
        want_bytes, got_bytes = a.read(), b.read()
    assert len(want_bytes) > 0 and got_bytes == want_bytes
