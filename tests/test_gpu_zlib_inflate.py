"""GPU: the zlib-framed inflate of csrc/bgzf_inflate.hip (rocco_hip_zlib_inflate: header check, the shared DEFLATE decoder,
Adler-32 in HIP, one wavefront per data block; DESIGN.md section 0 row f10, note (31)) against its host twin and against zlib
on the three stream lists of tests/bigwig_files.py, one call per list; past the grid cap; rows that do not fit; no blocks;
and the guard bytes between the slots."""
import struct
import zlib

import numpy as np
import pytest

import bigwig_files as bf

pytestmark = pytest.mark.gpu


def run_device(gpu, streams, label=""):
    """One call of `rocco_hip_zlib_inflate` over [(span, capacity, framing)] into a guarded buffer: equal to the host twin's
    statuses, `produced` and (for accepted blocks) bytes, which are verified against zlib.  Returns the report."""
    import torch

    from rocco_amd import bigwig

    comp, table, n_out = bf.table_of(streams)
    host_out = np.full(n_out, bf.GUARD_BYTE, dtype=np.uint8)
    host_status, host_produced, host_report = bigwig.zlib_inflate_blocks_host(comp, table, host_out)
    out = torch.full((n_out,), bf.GUARD_BYTE, dtype=torch.uint8, device=gpu)
    comp_t = torch.from_numpy(np.frombuffer(comp, dtype=np.uint8).copy()).to(gpu)
    status, produced, report = bigwig.zlib_inflate_blocks_device(comp_t, torch.from_numpy(table).to(gpu), out)
    status, produced, out = status.cpu().numpy(), produced.cpu().numpy(), out.cpu().numpy()
    assert np.array_equal(status, host_status) and np.array_equal(produced, host_produced) and report == host_report, label
    for k in np.nonzero(status == 0)[0].tolist():
        slot = int(table[k, 3])
        assert np.array_equal(out[slot: slot + int(produced[k])], host_out[slot: slot + int(produced[k])]), (label, k)
    assert report["block"] == bf.verify(streams, table, status, produced, out, label), label  # (zlib's verdicts; the guard bytes)
    return report


def test_valid_streams(gpu):
    assert run_device(gpu, [c[1:] for c in bf.valid_streams()], "valid")["block"] == -1


def test_corrupt_streams(gpu):
    cases = bf.corrupt_streams()
    sound = bf.valid_streams()[0][1:]
    report = run_device(gpu, [sound] + [c[1:4] for c in cases] + [sound], "corrupt")
    assert report["block"] == 1 and bf.status_class(report["status"]) == cases[0][4]
    # the report of a length error states what the block inflates to
    (k, case), = [(k, c) for k, c in enumerate(cases) if c[0] == "inflates to capacity + 1"]
    report = run_device(gpu, [sound, case[1:4]], "length")
    assert report == {"block": 1, "status": bf.ERR_LENGTH, "produced": case[2] + 1}


def test_mutated_streams(gpu):
    cases = bf.mutated_streams()
    run_device(gpu, [(span, capacity, 0) for span, capacity in cases], "mutations")


def test_every_workgroup_takes_a_second_block(gpu):
    """ROCCO_ZLIB_MAX_GRID + 3 one-item fixedStep sections, each a stream of its own: a block past the cap is the next turn of
    a workgroup that keeps its tables and its staging window in LDS.  Every third block is refused in a way of its own, so
    that a workgroup's second turn follows a first that ended half-way."""
    import torch

    from rocco_amd import bigwig

    cap = bigwig.zlib_shape()["max_grid"]
    assert cap == bigwig.ZLIB_MAX_GRID
    n = cap + 3
    period = []
    for k in range(12):
        raw = bf.section_bytes(bf.section(0, 3, bf.f32([k + 0.5]), start=50 * k, step=50, span=50))
        span = bf.zlib_stream(raw, (6, 0, "fixed", 9)[k % 4])
        if k % 3 == 1:
            span = (span[:-1] + bytes([span[-1] ^ 1]), span[:-6], bytes([span[0], span[1] ^ 1]) + span[2:], span[:-2])[k // 3]
        period.append((span, len(raw), 0))
    assert (cap % 12) % 3 != 0  # (a refused block's workgroup goes on with a sound one)
    want = [bf.expected_status(*row) for row in period]
    assert sorted({bf.status_class(s) for s, _ in want}) == ["accepted", "adler", "header", "stream", "truncated"]
    comp_one = b"".join(span for span, _, _ in period)
    lengths = np.asarray([len(span) for span, _, _ in period], dtype=np.int64)
    first_one = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    index = np.arange(n, dtype=np.int64)
    table = np.zeros((n, 5), dtype=np.int64)
    table[:, 0] = first_one[index % 12]  # (every row reads the one period of compressed bytes: loads may overlap, stores may not)
    table[:, 1] = table[:, 0] + lengths[index % 12]
    table[:, 2] = 28
    table[:, 3] = 32 * index
    comp_t = torch.from_numpy(np.frombuffer(comp_one, dtype=np.uint8).copy()).to(gpu)
    out = torch.full((32 * n,), bf.GUARD_BYTE, dtype=torch.uint8, device=gpu)
    status, produced, report = bigwig.zlib_inflate_blocks_device(comp_t, torch.from_numpy(table).to(gpu), out)
    assert np.array_equal(status.cpu().numpy(), np.asarray([s for s, _ in want], dtype=np.int32)[index % 12])
    assert report["block"] == 1 and report["status"] == want[1][0]
    out = out.cpu().numpy().reshape(n, 32)
    assert np.all(out[:, 28:] == bf.GUARD_BYTE)
    for k in range(12):
        if want[k][0] == 0:
            rows = out[k::12, :28]
            assert np.all(rows == np.frombuffer(want[k][1], dtype=np.uint8)), k
            assert np.all(produced.cpu().numpy()[k::12] == 28)


def test_rows_that_do_not_fit_and_no_blocks(gpu):
    import torch

    from rocco_amd import bigwig

    streams = [c[1:] for c in bf.valid_streams()[:3]]
    comp, table, n_out = bf.table_of(streams)
    comp_t = torch.from_numpy(np.frombuffer(comp, dtype=np.uint8).copy()).to(gpu)
    for column, value in ((0, -1), (1, len(comp) + 1), (2, 65537), (2, -1), (3, -1), (3, n_out), (4, 2), (0, int(table[1, 1]) + 1)):
        bad = table.copy()
        bad[1, column] = value
        out = torch.full((n_out,), bf.GUARD_BYTE, dtype=torch.uint8, device=gpu)
        status, produced, report = bigwig.zlib_inflate_blocks_device(comp_t, torch.from_numpy(bad).to(gpu), out)
        assert status.cpu().tolist() == [0, bf.ERR_TABLE, 0] and report == {"block": 1, "status": bf.ERR_TABLE, "produced": 0}, (column, value)
        slot, capacity = int(table[1, 3]), int(table[1, 2])
        assert bool((out[slot - bf.GUARD: slot + capacity + bf.GUARD] == bf.GUARD_BYTE).all()), (column, value)
    empty = torch.empty(0, dtype=torch.uint8, device=gpu)
    status, produced, report = bigwig.zlib_inflate_blocks_device(empty, torch.empty(0, dtype=torch.int64, device=gpu), empty)
    assert status.numel() == 0 and produced.numel() == 0 and report["block"] == -1
