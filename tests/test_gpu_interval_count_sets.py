"""Row f12 on the GPU: `rocco_hip_count_alignment_intervals_sets` (rocco_amd/csrc/interval_count.hip) -- the counting of
row f6 with several option sets and placed output in one launch series -- against the existing entry point
(`count_alignment_intervals_batch_device`, pinned to the reference's counter by tests/test_gpu_interval_counts.py) called
once per option set on the same synthetic records.  Integer counts: every comparison is exact.

Sizes come from `rocco_hip_count_intervals_shape`: F = 4 files and P intervals with P * F above `max_grid *
waves_per_group` work units (the counting launch's grid stride runs more than one turn), and a pile of more than
2 * `unit_records` candidates at one locus (pairs of several units add with atomicAdd, the others store)."""
import ctypes

import numpy as np
import pytest

import alignment_counts_expected as expected

pytestmark = pytest.mark.gpu
OPTION_SETS = [
    dict(one_read_per_bin=1, flag_exclude=0, min_mapping_quality=10),   # the peaks of raw_count_matrix
    dict(one_read_per_bin=1, flag_exclude=4, min_mapping_quality=10),   # the null regions
    dict(one_read_per_bin=1, paired_end_mode=1, read_length=50, flag_exclude=3844, min_mapping_quality=10),
    dict(one_read_per_bin=0, extend_bp=150, shift_forward_strand53=4, shift_reverse_strand53=5, flag_exclude=3844),
]
POISON = -77
F = 4
PILE = 30000


@pytest.fixture(scope="module")
def shape(gpu):
    from rocco_amd.readtracks import count_intervals_shape

    return count_intervals_shape()


def to_records(fields):
    from rocco_amd.readtracks import AlignmentRecords

    return AlignmentRecords(*fields)


def with_pile(fields, depth, rng):
    """`fields` with `depth` more 50 bp records on PILE (every mapping quality, some unmapped), in coordinate order."""
    pos = np.concatenate([fields[0], np.full(depth, PILE, dtype=np.int32)])
    extra = (np.full(depth, PILE + 50, dtype=np.int32), np.zeros(depth, np.int32),
             np.where(rng.random(depth) < 0.1, 4, 0).astype(np.uint16), rng.integers(0, 61, size=depth).astype(np.uint8),
             np.ones(depth, np.uint8))
    order = np.argsort(pos, kind="stable")
    return (pos[order],) + tuple(np.concatenate([a, b])[order] for a, b in zip(fields[1:], extra))


@pytest.fixture(scope="module")
def case(shape):
    """Four files over the contigs a (dense, with the pile), b (one file's track empty) and e (no records in any file);
    P intervals with candidates nearly everywhere, some on the pile, some on e."""
    rng = np.random.default_rng(1212)
    unit = shape["unit_records"]
    none = tuple(np.zeros(0, dtype=d) for d in (np.int32, np.int32, np.int32, np.uint16, np.uint8, np.uint8))
    files = []
    for f in range(F):
        a = with_pile(expected.random_records(rng, 9000 + 500 * f, 60000), 2 * unit + 40 + 300 * f, rng)
        b = none if f == 2 else expected.random_records(rng, 2500, 25000)
        files.append({"a": a, "b": b, "e": none})
    P = shape["max_grid"] * shape["waves_per_group"] // F + 300
    contigs = rng.choice(["a", "a", "a", "b"], size=P)
    limit = np.where(contigs == "a", 59000, 24000)
    starts = (rng.random(P) * limit).astype(np.int64)
    ends = starts + rng.integers(150, 900, size=P)
    cut = [(PILE, PILE + 1), (PILE - 200, PILE + 25), (PILE + 49, PILE + 50), (PILE + 50, PILE + 60), (PILE - 5000, PILE + 5000), (0, 60000)]
    for k, (s, e) in enumerate(cut):
        contigs[7 * k + 3], starts[7 * k + 3], ends[7 * k + 3] = "a", s, e
    for k in range(12):  # the contig without records, and the file without a track on b
        contigs[11 * k + 60] = "e"
    assert P * F > shape["max_grid"] * shape["waves_per_group"]
    return {"files": [{c: to_records(v) for c, v in by.items()} for by in files], "contigs": contigs, "starts": starts, "ends": ends, "P": P}


@pytest.fixture(scope="module")
def per_set(gpu, case):
    """[S][P, F]: every interval under every option set by the existing entry point, one call per set; computed once."""
    from rocco_amd.readtracks import count_alignment_intervals_batch_device

    return [count_alignment_intervals_batch_device(case["files"], case["contigs"], case["starts"], case["ends"], **options).cpu().numpy()
            for options in OPTION_SETS]


def placed(case, S, gpu, col0=2, files=None):
    """The sets call with the intervals' sets interleaved (p % S) and rows reversed and strided inside a larger, poisoned
    `out`: (out as a host array, the rows)."""
    import torch

    from rocco_amd.readtracks import count_alignment_intervals_sets_device

    P = case["P"]
    rows = 2 * (P - 1 - np.arange(P)) + 1
    out = torch.full((2 * P + 3, F + 3), POISON, dtype=torch.int32, device=gpu)
    for f0, f1, at in files or [(0, F, col0)]:
        count_alignment_intervals_sets_device(case["files"][f0:f1], case["contigs"], case["starts"], case["ends"], np.arange(P) % S,
                                              OPTION_SETS[:S], rows, out, col0=at)
    return out.cpu().numpy(), rows


@pytest.mark.parametrize("S", [1, 2, 4])
def test_sets_call_equals_one_call_per_set(gpu, shape, case, per_set, S):
    P, unit = case["P"], shape["unit_records"]
    sets = np.arange(P) % S
    want = np.stack([per_set[s][p] for p, s in enumerate(sets)])
    # what the case is for: more units than one turn of the grid holds, pairs of several units, addressed zeros
    assert np.count_nonzero(per_set[0]) > shape["max_grid"] * shape["waves_per_group"]
    assert int(want.max()) > 2 * unit and np.count_nonzero(want == 0) > 40 and np.count_nonzero((want > 0) & (want < unit)) > 1000
    got, rows = placed(case, S, gpu)
    assert np.array_equal(got[rows, 2:2 + F], want)
    untouched = np.ones(got.shape, dtype=bool)
    untouched[rows[:, None], np.arange(2, 2 + F)[None, :]] = False
    assert np.all(got[untouched] == POISON) and np.count_nonzero(untouched) == got.size - P * F
    if S > 1:  # the sets differ on these records: a call that ignored the set ids would not pass
        assert any(not np.array_equal(per_set[0], per_set[s]) for s in range(1, S))


def test_two_column_groups_equal_one_call(gpu, case):
    together, rows = placed(case, 2, gpu, col0=1)
    in_groups, _ = placed(case, 2, gpu, files=[(0, 1, 1), (1, F, 2)])
    assert together.tobytes() == in_groups.tobytes() and np.all(together[rows, 1:1 + F] != POISON)


def raw_call(gpu, n_sets, set_ids, rows, out, col0, n_files=2):
    """The entry point itself over two short tracks and three intervals: (return code, track facts)."""
    import torch

    from rocco_amd import _native
    from rocco_amd import dp
    from rocco_amd.readtracks import CountOptions, _count_options, _record_args

    rng = np.random.default_rng(4)
    tracks = [to_records(expected.random_records(rng, 600, 5000)) for _ in range(n_files)]
    cat, rec_offsets, dev = _record_args(tracks, dev=gpu)
    opts = (CountOptions * 5)(*[_count_options(0, **OPTION_SETS[s % 2]) for s in range(5)])
    arrays = [torch.tensor(v, dtype=t, device=dev) for v, t in ((set_ids, torch.int32), ([0, 0, 0], torch.int32), ([0, 100, 2000], torch.int32),
                                                                ([5000, 900, 2600], torch.int32), (rows, torch.int64))]
    facts = (ctypes.c_int * (2 * n_files))()
    rc = _native.load().rocco_hip_count_alignment_intervals_sets(
        _native.solver_for(dev.index).handle, cat.pos.data_ptr(), cat.end.data_ptr(), cat.isize.data_ptr(), cat.flag.data_ptr(),
        cat.mapq.data_ptr(), cat.mate_same.data_ptr(), rec_offsets, n_files, 1, ctypes.cast(opts, ctypes.c_void_p), n_sets,
        arrays[0].data_ptr(), arrays[1].data_ptr(), arrays[2].data_ptr(), arrays[3].data_ptr(), arrays[4].data_ptr(), 3, out.data_ptr(),
        int(out.shape[0]), int(out.shape[1]), col0, facts, dp._stream_ptr(out))
    return rc, list(facts)


def test_invalid_arguments_are_einval(gpu):
    import torch

    from rocco_amd import _native

    def fresh():
        return torch.full((6, 4), POISON, dtype=torch.int32, device=gpu)

    out = fresh()
    rc, _ = raw_call(gpu, 2, [0, 1, 0], [4, 0, 2], out, 1)
    assert rc == _native.OK
    good = out.cpu().numpy()
    assert np.all(good[[4, 0, 2], 1:3] > 0) and np.count_nonzero(good == POISON) == 24 - 6
    for n_sets, col0 in ((5, 1), (0, 1), (2, 3)):  # too many sets, none, col0 + F > stride: refused before anything is queued
        out = fresh()
        assert raw_call(gpu, n_sets, [0, 1, 0], [4, 0, 2], out, col0)[0] == _native.EINVAL
        assert bool((out == POISON).all())
    for set_ids, rows in (([0, 2, 0], [4, 0, 2]), ([0, -1, 0], [4, 0, 2]), ([0, 1, 0], [4, 6, 2]), ([0, 1, 0], [4, -1, 2])):
        out = fresh()
        assert raw_call(gpu, 2, set_ids, rows, out, 1)[0] == _native.EINVAL, (set_ids, rows)
        got = out.cpu().numpy()
        # no cell of the offending interval is written (its row, where it has one, keeps the poison); the others' are
        assert np.array_equal(got[[4, 2]], good[[4, 2]]) and np.all(got[[0, 1, 3, 5]] == POISON)


def test_python_checks_rows_and_sets(gpu, case):
    import torch

    from rocco_amd.readtracks import count_alignment_intervals_sets_device as call

    out = torch.full((4, F), POISON, dtype=torch.int32, device=gpu)
    args = (case["files"], ["a", "b"], [0, 10], [100, 500])
    with pytest.raises(ValueError, match="distinct"):
        call(*args, [0, 0], OPTION_SETS[:1], [1, 1], out)
    with pytest.raises(ValueError, match="outside"):
        call(*args, [0, 0], OPTION_SETS[:1], [1, 4], out)
    with pytest.raises(ValueError, match="names no option set"):
        call(*args, [0, 1], OPTION_SETS[:1], [1, 2], out)
    with pytest.raises(ValueError, match="option sets"):
        call(*args, [0, 1], OPTION_SETS + OPTION_SETS[:1], [1, 2], out)
    with pytest.raises(ValueError, match="do not fit"):
        call(*args, [0, 0], OPTION_SETS[:1], [1, 2], out, col0=1)
    assert bool((out == POISON).all())


def test_unsorted_track_is_refused(gpu):
    import torch

    from rocco_amd.readtracks import count_alignment_intervals_sets_device as call

    track = expected.random_records(np.random.default_rng(5), 40000, 300000)
    shuffled = [a.copy() for a in track]
    shuffled[0][[20000, 20001]] = shuffled[0][[20001, 20000]] + np.array([5, -5], dtype=np.int32)
    assert shuffled[0][20000] > shuffled[0][20001]
    files = [{"a": to_records(track), "b": to_records(track)}, {"a": to_records(track), "b": to_records(tuple(shuffled))}]
    out = torch.zeros((2, 3), dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError, match="file 1 on b are not in coordinate order"):
        call(files, ["a", "b"], [0, 10], [100, 500], [0, 1], OPTION_SETS[:2], [0, 1], out)
    with pytest.raises(ValueError, match="file 2 on b are not in coordinate order"):  # (named by its column)
        call(files[1:], ["a", "b"], [0, 10], [100, 500], [0, 1], OPTION_SETS[:2], [0, 1], out, col0=2)
    call(files[:1], ["a", "b"], [0, 10], [100, 500], [0, 1], OPTION_SETS[:2], [0, 1], out)  # the sorted file alone passes
