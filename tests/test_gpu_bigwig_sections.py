"""GPU: the section decode of bigWig files (note (31); csrc/bigwig_sections.hip over the rules of
csrc/bigwig_sections.h): the two device entry points against the host twin and against the second reader of tests/bigwig_files.py on every
file of both case lists, by bit pattern, in both inflate modes and for K files in one batch; hand-built slots past one launch's first
turn, sized from `rocco_hip_bigwig_sections_shape`; guard elements behind the outputs and poisoned tails behind `produced`; what the
entry points refuse; and the refusals of a section as `read_bigwig_intervals` words them."""
import ctypes
import os
import re
import struct
import zlib

import numpy as np
import pytest

import bigwig_files as bf
import bigwig_sections_cases as cases

pytestmark = pytest.mark.gpu
NAMES = ("starts", "ends", "values")


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    return cases.write_all(tmp_path_factory.mktemp("bigwig_sections_gpu"))


@pytest.fixture(scope="module")
def inputs(written):
    return cases.file_inputs(written)


def on_device(gpu, slots, table, produced):
    import torch

    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (slots, table.reshape(-1), produced))


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return a.view(np.uint64)


def same(got, expected):
    starts, ends, bits32 = expected
    return np.array_equal(got["starts"].cpu().numpy(), starts) and np.array_equal(got["ends"].cpu().numpy(), ends) and \
        np.array_equal(bits(got["values"]), cases.widened_bits(bits32))


def test_device_against_host_twin_and_second_reader(gpu, inputs):
    import torch

    from rocco_amd import bigwig

    seen = 0
    for label, sections, tid, length, expected in inputs:
        slots, table, produced = cases.layout(sections, tight=False)
        files = ([0, len(sections)], [tid], [length])
        host = bigwig.decode_sections_host(slots, table, produced, *files)
        got = bigwig.decode_sections_device(*on_device(gpu, slots, table, produced), *files)
        assert got["report"] == host["report"] and got["report"]["block"] == -1, label
        assert got["status"].cpu().numpy().tolist() == host["status"].tolist() and got["file_offsets"].tolist() == host["file_offsets"].tolist(), label
        assert got["starts"].dtype == torch.int64 and got["ends"].dtype == torch.int64 and got["values"].dtype == torch.float64
        assert same(got, expected) and all(np.array_equal(bits(got[k]), bits(host[k])) for k in NAMES), label
        seen += expected[0].size
    assert seen > 9000


def test_read_bigwig_intervals_in_both_inflate_modes(gpu, written):
    from rocco_amd import bigwig

    for label, path, record, chromosomes in written:
        for chromosome in chromosomes:
            expected = bf.expected_intervals(path, chromosome)
            for mode in ("device", "host"):
                if mode == "device" and record["uncompressBufSize"] > 65536:
                    continue
                got = bigwig.read_bigwig_intervals(path, chromosome, device=gpu, inflate=mode)
                if expected is None:
                    assert got is None, (label, chromosome)
                else:
                    assert same(dict(zip(NAMES, got)), bf.as_arrays(expected)) and got[0].device == gpu, (label, chromosome, mode)


def test_k_files_in_one_batch(gpu, written):
    from rocco_amd import bigwig

    wanted = [(path, chromosomes[0]) for _, path, record, chromosomes in written if record["uncompressBufSize"] <= 65536]
    wanted.append((wanted[0][0], "chrAbsent"))
    assert len(wanted) >= 20
    for mode in ("device", "host"):
        batch = bigwig.read_bigwig_intervals_batch(wanted, device=gpu, inflate=mode)
        assert batch[-1] is None and sum(int(b[0].shape[0]) for b in batch[:-1]) > 5000
        for (path, chromosome), got in zip(wanted[:-1], batch[:-1]):
            alone = bigwig.read_bigwig_intervals(path, chromosome, device=gpu, inflate=mode)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, alone)), (path, mode)
            assert same(dict(zip(NAMES, got)), bf.as_arrays(bf.expected_intervals(path, chromosome))), (path, mode)


def many_small_sections(n):
    """n stored fixedStep sections of 1 or 2 items each in slots of 32 bytes, built as arrays: (slots, table, produced, expected)."""
    index = np.arange(n, dtype=np.int64)
    count = 1 + index % 2
    rows = np.zeros(n, dtype=np.dtype([("chrom", "<u4"), ("start", "<u4"), ("end", "<u4"), ("step", "<u4"), ("span", "<u4"), ("type", "u1"),
                                       ("reserved", "u1"), ("count", "<u2"), ("v0", "<f4"), ("v1", "<f4")]))
    rows["start"], rows["end"], rows["step"], rows["span"], rows["type"], rows["count"] = 200 * index, 200 * index + 100, 50, 50, 3, count
    rows["v0"], rows["v1"] = index % 1000 + 0.25, -(index % 1000) - 0.5
    slots = rows.view(np.uint8).reshape(n, 32).copy()
    slots[count == 1, 28:] = cases.POISON  # (behind `produced`)
    table = np.zeros((n, 5), dtype=np.int64)
    table[:, 2], table[:, 3] = 32, 32 * index
    item = np.repeat(index, count)
    second = np.concatenate([[False], item[1:] == item[:-1]])
    starts = 200 * item + 50 * second
    values = np.where(second, rows["v1"][item], rows["v0"][item]).astype(np.float32)
    return slots.reshape(-1), table, 24 + 4 * count, (starts, starts + 50, values.view(np.uint32))


def test_every_workgroup_takes_a_second_block(gpu):
    """grid cap + 3 sections: block i + cap is the next turn of block i's workgroup."""
    from rocco_amd import bigwig

    shape = bigwig.sections_shape()
    n = shape["max_grid"] + 3
    slots, table, produced, expected = many_small_sections(n)
    assert 2_000_000 < slots.size < 3_000_000
    files = ([0, 5, 5, n], [0, 0, 0], [10 ** 9, 10 ** 9, 10 ** 9])  # (three files, the second without a block)
    got = bigwig.decode_sections_device(*on_device(gpu, slots, table, produced), *files)
    assert got["report"] == {"block": -1, "status": 0, "produced": expected[0].size} and same(got, expected)
    assert got["file_offsets"].tolist() == [0, 7, 7, expected[0].size]
    host = bigwig.decode_sections_host(slots, table, produced, *files)
    assert all(np.array_equal(bits(got[k]), bits(host[k])) for k in NAMES)


def test_a_section_of_the_headers_maximum_of_items(gpu):
    """65 535 fixedStep items: 1 024 turns of one wavefront; the chromosome ends inside the section."""
    from rocco_amd import bigwig

    values = bf.f32(np.arange(65535) % 977 + 0.5)
    data = bf.section_bytes(bf.section(0, 3, values, start=1000, step=3, span=2))
    length = 1000 + 3 * 60001 + 1  # (item 60 001 starts one below the length, item 60 002 is dropped)
    slots, table, produced = cases.layout([data, data[:24 + 4 * 100]], tight=False)  # (the second: cut short of its count)
    got = bigwig.decode_sections_device(*on_device(gpu, slots, table, produced), [0, 2], [0], [length])
    assert got["report"] == {"block": 1, "status": cases.ERR_ITEMS, "produced": 60002} and got["starts"] is None
    got = bigwig.decode_sections_device(*on_device(gpu, *cases.layout([data], tight=False)), [0, 1], [0], [length])
    starts = 1000 + 3 * np.arange(60002, dtype=np.int64)
    assert same(got, (starts, starts + 2, values[:60002].view(np.uint32)))


def test_dropped_items_on_both_sides_of_a_turn_boundary(gpu):
    from rocco_amd import bigwig

    threads = bigwig.sections_shape()["threads"]
    length, n = 100000, 3 * threads + 5
    for gone in ([threads - 1, threads], [threads - 2, threads - 1, threads, threads + 1, 2 * threads], list(range(threads)), list(range(threads, 2 * threads)),
                 [0, n - 1], list(range(n))):
        var = [(length + j if j in gone else 10 * j, np.float32(j + 0.5)) for j in range(n)]
        bed = [(10 * j, 0 if j in gone else 10 * j + 7, np.float32(-j)) for j in range(n)]  # (an end of 0: dropped on the other rule)
        sections = [bf.section_bytes(bf.section(0, 2, var, span=10)), bf.section_bytes(bf.section(0, 1, bed))]
        slots, table, produced = cases.layout(sections, tight=False)
        got = bigwig.decode_sections_device(*on_device(gpu, slots, table, produced), [0, 2], [0], [length])
        kept = [j for j in range(n) if j not in gone]
        want = [(10 * j, 10 * j + 10, np.float32(j + 0.5)) for j in kept] + [(10 * j, 10 * j + 7, np.float32(-j)) for j in kept]
        assert got["report"]["block"] == -1 and same(got, bf.as_arrays(want)), gone


def test_guard_elements_and_poisoned_tails(gpu, inputs):
    """The outputs lie in front of 64 guard elements each, which stay as they were; the bytes of every slot behind `produced` are
    poison in one run and zeros in the other, and the results are the same."""
    import torch

    from rocco_amd import bigwig

    label, sections, tid, length, expected = next(entry for entry in inputs if entry[0].startswith("turns.bw"))
    files = ([0, len(sections)], [tid], [length])
    results = []
    for poison in (True, False):
        slots, table, produced = cases.layout(sections, tight=False, poison=poison)
        tensors = on_device(gpu, slots, table, produced)
        status_t, block_first_t, offsets, report = bigwig.sections_facts_device(*tensors, *files)
        total = report["produced"]
        assert report["block"] == -1 and total == expected[0].size and int(block_first_t[-1]) == total
        whole = [torch.full((total + 64,), -77, dtype=torch.int64, device=gpu), torch.full((total + 64,), -77, dtype=torch.int64, device=gpu),
                 torch.full((total + 64,), -77.0, dtype=torch.float64, device=gpu)]
        bigwig.sections_emit_device(*tensors, *files, block_first_t, total, *(w[:total] for w in whole))
        torch.cuda.synchronize()
        assert all(bool((w[total:] == -77).all()) for w in whole), "an element behind an output was written"
        results.append(dict(zip(NAMES, (w[:total] for w in whole))))
        assert same(results[-1], expected)
    assert all(np.array_equal(bits(results[0][k]), bits(results[1][k])) for k in NAMES)


def test_what_the_device_entry_points_refuse(gpu):
    import torch

    from rocco_amd import _native, bigwig
    from rocco_amd import dp

    sections = [bf.section_bytes(s) for s in bf.fixed_sections(0, 2, 5, seed=4)]
    slots, table, produced = cases.layout(sections, tight=False)
    files = ([0, 2], [0], [10 ** 7])
    for column, value in ((3, slots.size - 10), (3, -8), (2, -1), (2, slots.size + 1)):  # a row outside the slots: nothing of it is read
        bad = table.copy()
        bad[1, column] = value
        got = bigwig.decode_sections_device(*on_device(gpu, slots, bad, produced), *files)
        assert got["status"].tolist() == [0, cases.ERR_TABLE] and got["report"] == {"block": 1, "status": cases.ERR_TABLE, "produced": 5}
    got = bigwig.decode_sections_device(*on_device(gpu, slots, table, np.asarray([int(table[0, 2]) + 1, produced[1]])), *files)  # produced > capacity
    assert got["status"].tolist() == [cases.ERR_TABLE, 0] and got["starts"] is None
    tensors = on_device(gpu, slots, table, produced)
    with pytest.raises(ValueError, match="rocco_hip_bigwig_sections_facts"):
        bigwig.sections_facts_device(*tensors, [0, 1], [0], [10 ** 7])
    status_t, block_first_t, offsets, report = bigwig.sections_facts_device(*tensors, *files)
    assert report == {"block": -1, "status": 0, "produced": 10}
    out = [torch.full((74,), -7, dtype=torch.int64, device=gpu), torch.full((74,), -7, dtype=torch.int64, device=gpu),
           torch.full((74,), -7.0, dtype=torch.float64, device=gpu)]
    for short in range(3):  # an output smaller than the total
        views = [a[:9] if k == short else a[:10] for k, a in enumerate(out)]
        with pytest.raises(ValueError, match="rocco_hip_bigwig_sections_emit"):
            bigwig.sections_emit_device(*tensors, *files, block_first_t, 10, *views)
    with pytest.raises(ValueError, match="rocco_hip_bigwig_sections_emit"):  # block_first shorter than n + 1
        bigwig.sections_emit_device(*tensors, *files, block_first_t[:2], 10, *(a[:10] for a in out))
    # a null pointer with a size: the C entry point itself (the Python side never hands one over)
    lib, first, ids, lengths = _native.load(), *bigwig._file_arrays(*files)
    solver, stream = _native.solver_for(gpu.index).handle, dp._stream_ptr(tensors[0])
    for missing in range(3):
        pointers = [None if k == missing else a.data_ptr() for k, a in enumerate(out)]
        rc = lib.rocco_hip_bigwig_sections_emit(solver, tensors[0].data_ptr(), slots.size, tensors[1].data_ptr(), tensors[2].data_ptr(), 2,
                                                bigwig._ll(first), bigwig._ll(ids), bigwig._ll(lengths), 1, block_first_t.data_ptr(), 3, 10,
                                                pointers[0], 10, pointers[1], 10, pointers[2], 10, stream)
        assert rc == _native.EINVAL, missing
    back = (ctypes.c_longlong * 4)()
    rc = lib.rocco_hip_bigwig_sections_facts(solver, None, slots.size, tensors[1].data_ptr(), tensors[2].data_ptr(), 2, bigwig._ll(first),
                                             bigwig._ll(ids), bigwig._ll(lengths), 1, status_t.data_ptr(), 2, block_first_t.data_ptr(), 3,
                                             bigwig._ll(offsets), back, stream)
    assert rc == _native.EINVAL
    torch.cuda.synchronize()
    assert all(bool((a == -7).all()) for a in out)  # (a refused call launches nothing)
    bigwig.sections_emit_device(*tensors, *files, block_first_t, 10, *(a[:10] for a in out))
    assert out[0][:10].tolist() == [50 * j for j in range(10)] and all(bool((a[10:] == -7).all()) for a in out)
    # a total of zero launches nothing, whatever the outputs are
    empty = [torch.empty(0, dtype=torch.int64, device=gpu), torch.empty(0, dtype=torch.int64, device=gpu), torch.empty(0, dtype=torch.float64, device=gpu)]
    bigwig.sections_emit_device(*tensors, *files, block_first_t, 0, *empty)


def refused_file(directory, name, bad, buf_size=None):
    """A file of three blocks whose second is `bad`: a section dict, or the raw bytes of a section (compressed here)."""
    sound = bf.fixed_sections(0, 3, 20, seed=5)
    if isinstance(bad, bytes):
        bad = dict(sound[1], payload=bad if buf_size == 0 else zlib.compress(bad))
    path = os.path.join(str(directory), name)
    return path, bf.write_bigwig(path, [("chr1", 10 ** 7)], [sound[0], bad, sound[2]], buf_size=buf_size, block_size=2)


def test_refused_sections_through_read_bigwig_intervals(gpu, tmp_path):
    from rocco_amd import bigwig

    sound = bf.fixed_sections(0, 3, 20, seed=5)[1]
    files = {
        "short": (cases.header(count=0)[:23], "the section is shorter than its 24-byte header"),
        "short_stored": (cases.header(count=0)[:23], "the section is shorter than its 24-byte header"),
        "type0": (dict(sound, header_type=0), "the section's type is not 1 (bedGraph), 2 (variableStep) or 3 (fixedStep)"),
        "type4": (dict(sound, header_type=4), "the section's type is not 1 (bedGraph), 2 (variableStep) or 3 (fixedStep)"),
        "count": (dict(sound, item_count=21), "the section's header counts more items than its bytes hold (libBigWig would read past the section)"),
        "wrap": (bf.section(0, 2, [(100, np.float32(1)), (2 ** 32 - 16, np.float32(2))], span=16, leaf=(0, 1000, 0, 2000)),
                 "an item of the section ends beyond 4294967295 (libBigWig would wrap around)"),
    }
    for name, (bad, words) in files.items():
        path, record = refused_file(tmp_path, name + ".bw", bad, buf_size=0 if name.endswith("stored") else None)
        pattern = re.escape(f"{path}: bigWig data block 1 at file offset {record['blocks'][1][0]}: {words}")
        said = []
        for mode in ("device", "host"):
            with pytest.raises(ValueError, match=pattern) as info:
                bigwig.read_bigwig_intervals(path, "chr1", device=gpu, inflate=mode)
            said.append(str(info.value))
        assert said[0] == said[1], name
        with pytest.raises(ValueError, match=pattern):  # (in a batch, behind another file's blocks: the file's own block index)
            bigwig.read_bigwig_intervals_batch([(refused_file(tmp_path, "sound.bw", sound)[0], "chr1"), (path, "chr1")], device=gpu)
        if name == "wrap":
            with pytest.raises(OverflowError):
                bf.expected_intervals(path, "chr1")
