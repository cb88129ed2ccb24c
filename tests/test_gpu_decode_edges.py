"""GPU: the run decode (rocco_amd/csrc/decode.hip) at its structural edges, every case of tests/decode_cases.py through
all three entry points (decode_runs_device, decode_runs_batch_device, decode_runs_table_device), exactly.

What the cases reach is asserted without a device in tests/test_decode_cases_host.py: the scan's carry over two and
three trips, runs that start at, end at and cross lane, wavefront, tile and trip boundaries, lanes of 8 starts, tables of
one, two and more strides of the to-host kernel with odd and even row totals, the last locus.  Here in addition:
solutions that are not 16-byte aligned (a 1-D slice is contiguous, so the kernels get the pointer as it is and every lane
takes the byte loop of `lane_bits`), other dtypes (selected means > 0.5, rocco/rocco.py:183), the capacity guards through
the C ABI with sentinel-filled buffers, units of any sign and size, and run-to-run identity.

Decode is integer work: every comparison is exact."""
import ctypes

import numpy as np
import pytest

import decode_cases as dc

pytestmark = pytest.mark.gpu

CALLS = dc.batches()
SENTINEL = -0x5A5A5A5A5A5A5A5B
GUARD = 64


@pytest.fixture(scope="module")
def built():
    """name -> (z, begins, ends); computed once, never modified."""
    out = {}
    for name, _n, builder in dc.cases():
        z = builder()
        out[name] = (z,) + dc.expected_runs(z)
    return out


def _unit(i):
    """Units of either sign, most of them beyond 32 bits."""
    return (-1) ** i * (i * ((1 << 33) + 12345) + 7)


def _same_runs(got_b, got_e, want_b, want_e, what):
    got_b, got_e = np.asarray(got_b), np.asarray(got_e)
    assert got_b.shape == want_b.shape and got_e.shape == want_e.shape, (what, got_b.shape, got_e.shape, want_b.shape)
    for got, want, side in ((got_b, want_b, "begin"), (got_e, want_e, "end")):
        if not np.array_equal(got, want):
            at = int(np.flatnonzero(got != want)[0])
            raise AssertionError(f"{what}: {side}[{at}] is {int(got[at])}, expected {int(want[at])} ({want.size} runs)")


def _upload(call, built, gpu):
    import torch

    return [torch.from_numpy(built[name][0]).to(gpu) for name, _n, _b in call]


# ---- every case, three forms ----
@pytest.mark.parametrize("ci", range(len(CALLS)))
def test_single_form_decodes_every_case(gpu, built, ci):
    from rocco_amd import rocco as impl

    for (name, _n, _b), sol in zip(CALLS[ci], _upload(CALLS[ci], built, gpu)):
        begin_t, end_t = impl.decode_runs_device(sol)
        _same_runs(begin_t.cpu().numpy(), end_t.cpu().numpy(), built[name][1], built[name][2], name)


@pytest.mark.parametrize("ci", range(len(CALLS)))
def test_batch_form_decodes_every_case(gpu, built, ci):
    from rocco_amd import rocco as impl

    call = CALLS[ci]
    if any(dc.scan_trips(n) > 1 for _name, n, _b in call):
        assert call[0][1] < dc.TRIP  # the multi-trip tasks do not begin at tile 0 of the launch
    pairs = impl.decode_runs_batch_device(_upload(call, built, gpu))
    assert len(pairs) == len(call)
    for (name, _n, _b), (begin_t, end_t) in zip(call, pairs):
        _same_runs(begin_t.cpu().numpy(), end_t.cpu().numpy(), built[name][1], built[name][2], name)


@pytest.mark.parametrize("ci", range(len(CALLS)))
def test_table_form_decodes_every_case(gpu, built, ci):
    from rocco_amd import rocco as impl

    call = CALLS[ci]
    units = [_unit(i) for i in range(len(call))]
    table_t, offsets, host = impl.decode_runs_table_device(_upload(call, built, gpu), units=units)
    want_offsets = np.concatenate([[0], np.cumsum([built[name][1].size for name, _n, _b in call])]).tolist()
    assert offsets == want_offsets
    table = table_t.cpu().numpy()
    assert table.shape == host.shape == (want_offsets[-1], 3)
    assert np.array_equal(host, table)
    for i, (name, _n, _b) in enumerate(call):
        rows = table[offsets[i]:offsets[i + 1]]
        assert np.all(rows[:, 0] == units[i]), name
        _same_runs(rows[:, 1], rows[:, 2], built[name][1], built[name][2], name)


# ---- solutions that are not 16-byte aligned ----
MISALIGNED_BASES = (dc.TILE + 33, 2 * dc.TILE + 16)


def _misaligned_base(nb):
    rng = np.random.default_rng(4000 + nb)
    z = (rng.random(nb) < 0.5).astype(np.uint8)
    z[100:164:2], z[101:164:2] = 1, 0          # a 1010 patch
    z[:20] = 1                                  # every view starts inside a run
    z[-20:] = 1                                 # and ends in one (the view's last locus is never emitted)
    z[dc.TILE - 8:dc.TILE + 24] = 1             # a run over the tile boundary of every view
    z[z != 0] = rng.choice(np.array([1, 2, 0x80, 0xFF], dtype=np.uint8), size=int(np.count_nonzero(z)))
    return z


def _views(gpu, nb, ks):
    import torch

    z = _misaligned_base(nb)
    base_t = torch.from_numpy(z).to(gpu)
    assert base_t.data_ptr() % 16 == 0
    out = []
    for k in ks:
        view = base_t[k:]
        assert view.data_ptr() % 16 == k and view.is_contiguous() and view.contiguous().data_ptr() == view.data_ptr()
        out.append((view, dc.expected_runs(z[k:])))
    return base_t, out


@pytest.mark.parametrize("k", range(1, 16))
def test_misaligned_solution_three_forms(gpu, k):
    from rocco_amd import rocco as impl

    for nb in MISALIGNED_BASES:
        _base_t, [(view, (want_b, want_e))] = _views(gpu, nb, [k])
        assert want_b.size > 100
        what = f"base {nb} k={k}"
        begin_t, end_t = impl.decode_runs_device(view)
        _same_runs(begin_t.cpu().numpy(), end_t.cpu().numpy(), want_b, want_e, what + " single")
        [(begin_t, end_t)] = impl.decode_runs_batch_device([view])
        _same_runs(begin_t.cpu().numpy(), end_t.cpu().numpy(), want_b, want_e, what + " batch")
        table_t, offsets, host = impl.decode_runs_table_device([view], units=[-k])
        assert offsets == [0, want_b.size] and np.array_equal(host, table_t.cpu().numpy()) and np.all(host[:, 0] == -k)
        _same_runs(host[:, 1], host[:, 2], want_b, want_e, what + " table")


def test_misaligned_and_aligned_solutions_in_one_call(gpu):
    from rocco_amd import rocco as impl

    _base_t, views = _views(gpu, MISALIGNED_BASES[0], range(1, 16))
    sols, wants = [], []
    for view, want in views:
        aligned = view.clone()
        assert aligned.data_ptr() % 16 == 0
        sols += [view, aligned]
        wants += [want, want]
    pairs = impl.decode_runs_batch_device(sols)
    table_t, offsets, host = impl.decode_runs_table_device(sols, units=list(range(len(sols))))
    assert np.array_equal(host, table_t.cpu().numpy())
    for i, ((begin_t, end_t), (want_b, want_e)) in enumerate(zip(pairs, wants)):
        _same_runs(begin_t.cpu().numpy(), end_t.cpu().numpy(), want_b, want_e, f"batch task {i}")
        rows = host[offsets[i]:offsets[i + 1]]
        assert np.all(rows[:, 0] == i)
        _same_runs(rows[:, 1], rows[:, 2], want_b, want_e, f"table task {i}")


# ---- other dtypes: selected means > 0.5 (rocco/rocco.py:183) ----
def _typed_solutions():
    n = dc.TILE + 3
    rng = np.random.default_rng(77)
    above = np.nextafter(0.5, 1.0)
    f = rng.choice(np.array([0.0, 0.5, above, np.nan, 2.0, 1.0, -1.0, np.nextafter(0.5, 0.0), np.inf, -np.inf]), size=n)
    f[:6] = [above, above, 0.5, np.nan, 2.0, 0.0]
    f[-3:] = [2.0, above, 1.0]  # a run into the last locus
    i = rng.choice(np.array([-1, 0, 1, 2, 1 << 40, -(1 << 40)], dtype=np.int64), size=n)
    b = rng.random(n) < 0.4
    return {"float64": f, "int64": i, "bool": b}


@pytest.mark.parametrize("kind", ["bool", "int64", "float64"])
def test_other_dtypes_select_above_one_half(gpu, oracle, kind):
    import torch
    from rocco_amd import rocco as impl

    x = _typed_solutions()[kind]
    n = x.shape[0]
    with np.errstate(invalid="ignore"):
        want_b, want_e = dc.expected_runs((x > 0.5).astype(np.uint8))
    assert want_b.size > 50
    x_t = torch.from_numpy(x).to(gpu)
    assert str(x_t.dtype) == "torch." + kind
    begin_t, end_t = impl.decode_runs_device(x_t)
    _same_runs(begin_t.cpu().numpy(), end_t.cpu().numpy(), want_b, want_e, kind)
    intervals = 1000 + 50 * np.arange(n, dtype=np.int64)
    want_recs = oracle.chrom_solution_records("chrT", intervals, x)
    assert [(s, e) for _c, s, e in want_recs] == list(zip(intervals[want_b].tolist(), intervals[want_e].tolist()))
    for given in (x, x_t, torch.from_numpy(x)):
        assert impl.chrom_solution_records("chrT", intervals, given) == want_recs


# ---- the capacity guards, through the C ABI ----
# Buffers hold the runs that exist plus GUARD elements and are filled with a sentinel; `capacity` is what the call is told.
# Everything from `capacity` on is guard: nothing there may change, however many runs the kernels find.
CAPACITY_CASES = ("alt10@4098", "rand@8194", "pair[4095,4096]@8193", "run[n-3,n)@8193#0x80")


def _capacities(count):
    return sorted({0, 1, count // 2, count - 1} - {-1, count})


def _native_handle(gpu):
    from rocco_amd import _native

    return _native, _native.load(), _native.solver_for(gpu.index).handle


@pytest.mark.parametrize("null_pointers", [False, True], ids=["buffers", "null"])
@pytest.mark.parametrize("name", CAPACITY_CASES)
def test_capacity_guard_single(gpu, built, name, null_pointers):
    import torch
    from rocco_amd import dp as _dp

    _native, lib, handle = _native_handle(gpu)
    z, want_b, want_e = built[name]
    count = want_b.size
    sol = torch.from_numpy(z).to(gpu)
    for cap in ([0] if null_pointers else _capacities(count)):
        begin_t = torch.full((count + GUARD,), SENTINEL, dtype=torch.int64, device=gpu)
        end_t = torch.full((count + GUARD,), SENTINEL, dtype=torch.int64, device=gpu)
        n_runs = ctypes.c_size_t(12345)
        _native.check(lib.rocco_hip_decode_runs(handle, sol.data_ptr(), z.size, None if null_pointers else begin_t.data_ptr(),
                                                None if null_pointers else end_t.data_ptr(), cap, ctypes.byref(n_runs),
                                                _dp._stream_ptr(sol)), "rocco_hip_decode_runs")
        assert n_runs.value == count, (name, cap)
        b, e = begin_t.cpu().numpy(), end_t.cpu().numpy()
        assert np.array_equal(b[:cap], want_b[:cap]) and np.array_equal(e[:cap], want_e[:cap]), (name, cap)
        assert np.all(b[cap:] == SENTINEL) and np.all(e[cap:] == SENTINEL), (name, cap)


def test_capacity_guard_batch(gpu, built):
    import torch
    from rocco_amd import dp as _dp

    _native, lib, handle = _native_handle(gpu)
    tasks = []  # (name, capacity, null pointers)
    for name in CAPACITY_CASES:
        count = built[name][1].size
        tasks += [(name, cap, False) for cap in _capacities(count)] + [(name, 0, True), (name, count + 5, False)]
    k = len(tasks)
    assert k <= dc.BATCH_MAX
    sols = [torch.from_numpy(built[name][0]).to(gpu) for name, _c, _z in tasks]
    room = [max(built[name][1].size, cap) + GUARD for name, cap, _z in tasks]
    begins = [torch.full((r,), SENTINEL, dtype=torch.int64, device=gpu) for r in room]
    ends = [torch.full((r,), SENTINEL, dtype=torch.int64, device=gpu) for r in room]
    n_runs = (ctypes.c_size_t * k)(*([12345] * k))
    _native.check(lib.rocco_hip_decode_runs_batch(
        handle, k, (ctypes.c_void_p * k)(*[s.data_ptr() for s in sols]), (ctypes.c_size_t * k)(*[s.shape[0] for s in sols]),
        (ctypes.c_void_p * k)(*[None if t[2] else b.data_ptr() for t, b in zip(tasks, begins)]),
        (ctypes.c_void_p * k)(*[None if t[2] else e.data_ptr() for t, e in zip(tasks, ends)]),
        (ctypes.c_size_t * k)(*[t[1] for t in tasks]), n_runs, _dp._stream_ptr(sols[0])), "rocco_hip_decode_runs_batch")
    for i, (name, cap, _null) in enumerate(tasks):
        _z, want_b, want_e = built[name]
        assert n_runs[i] == want_b.size, (name, cap)
        b, e = begins[i].cpu().numpy(), ends[i].cpu().numpy()
        kept = min(cap, want_b.size)
        assert np.array_equal(b[:kept], want_b[:kept]) and np.array_equal(e[:kept], want_e[:kept]), (name, cap)
        assert np.all(b[kept:] == SENTINEL) and np.all(e[kept:] == SENTINEL), (name, cap)


def _raw_table(gpu, sols, units, cap, total, null_table=False):
    import torch
    from rocco_amd import dp as _dp

    _native, lib, handle = _native_handle(gpu)
    k = len(sols)
    table_t = torch.full((max(total, cap) + GUARD, 3), SENTINEL, dtype=torch.int64, device=gpu)
    offsets = (ctypes.c_size_t * (k + 1))(*([12345] * (k + 1)))
    host_ptr = ctypes.c_void_p(0xDEAD0)
    _native.check(lib.rocco_hip_decode_runs_table(
        handle, k, (ctypes.c_void_p * k)(*[s.data_ptr() for s in sols]), (ctypes.c_size_t * k)(*[s.shape[0] for s in sols]),
        (ctypes.c_longlong * k)(*units), None if null_table else table_t.data_ptr(), cap, cap, offsets, ctypes.byref(host_ptr),
        _dp._stream_ptr(sols[0])), "rocco_hip_decode_runs_table")
    return table_t.cpu().numpy(), [int(v) for v in offsets], host_ptr.value


def test_capacity_guard_table(gpu, built):
    import torch

    names = list(CAPACITY_CASES)
    sols = [torch.from_numpy(built[name][0]).to(gpu) for name in names]
    units = [_unit(i + 3) for i in range(len(names))]
    want = np.concatenate([np.stack([np.full(built[name][1].size, u, dtype=np.int64), built[name][1], built[name][2]], axis=1)
                           for name, u in zip(names, units)])
    total = want.shape[0]
    want_offsets = np.concatenate([[0], np.cumsum([built[name][1].size for name in names])]).tolist()
    first = built[names[0]][1].size
    for cap in (0, 1, first - 1, first, first + 1, total - 1):
        table, offsets, host = _raw_table(gpu, sols, units, cap, total)
        assert offsets == want_offsets and offsets[-1] == total, cap
        assert host is None, cap  # NULL: the table did not fit
        assert np.array_equal(table[:cap], want[:cap]), cap
        assert np.all(table[cap:] == SENTINEL), cap
    table, offsets, host = _raw_table(gpu, sols, units, 0, total, null_table=True)
    assert offsets == want_offsets and host is None and np.all(table == SENTINEL)
    for cap in (total, total + 7):
        table, offsets, host = _raw_table(gpu, sols, units, cap, total)
        assert offsets == want_offsets and host, cap
        rows = np.frombuffer((ctypes.c_int64 * (3 * total)).from_address(host), dtype=np.int64).reshape(total, 3)
        assert np.array_equal(rows, want) and np.array_equal(table[:total], want) and np.all(table[total:] == SENTINEL), cap


# ---- units, determinism ----
def test_units_arrive_unchanged(gpu, built):
    import torch
    from rocco_amd import rocco as impl

    units = [-(1 << 63), -1, 0, (1 << 32), (1 << 32) + 1, -(1 << 32) - 1, (1 << 63) - 1]
    names = ["rand@34", "alt10@17", "single[16]@4098", "rand@4097", "ones@8194", "alt01@33", "pair[0,1]@8193"]
    sols = [torch.from_numpy(built[name][0]).to(gpu) for name in names]
    table_t, offsets, host = impl.decode_runs_table_device(sols, units=units)
    assert np.array_equal(host, table_t.cpu().numpy())
    for i, (name, unit) in enumerate(zip(names, units)):
        rows = host[offsets[i]:offsets[i + 1]]
        assert rows.shape[0] == built[name][1].size > 0 and np.all(rows[:, 0] == unit), name


def test_dense_decode_is_identical_run_to_run(gpu, built):
    import torch
    from rocco_amd import rocco as impl

    name = f"alt10@{dc.DENSE_N}"
    sol = torch.from_numpy(built[name][0]).to(gpu)
    first = impl.decode_runs_device(sol)
    again = impl.decode_runs_device(sol)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    t1 = impl.decode_runs_table_device([sol, sol], units=[5, -5])
    host1 = t1[2].copy()  # (a view of the solver's pinned buffer: the next decode overwrites it)
    t2 = impl.decode_runs_table_device([sol, sol], units=[5, -5])
    assert torch.equal(t1[0], t2[0]) and t1[1] == t2[1] and np.array_equal(host1, t2[2])
    assert np.array_equal(t1[0][:built[name][1].size, 1].cpu().numpy(), built[name][1])
