"""The barcode census on the device (note (35)): the kernels of csrc/barcode_census.hip through
`rocco_amd.fragments` and through the C ABI, against the Python statement of ``ccounts_getCellCount``'s rule
(tests/barcode_census_expected.py), the host twin and the reference's stored cell counts -- barcodes byte for byte, counts
``array_equal`` -- on every fixture file in both inflate modes and in slabs of one BGZF block, at the structural edges of the
kernels (sizes from `rocco_hip_barcode_census_shape`), under degenerate hash masks, from the smallest table through several
rehashes, and with guard elements behind every array a kernel writes.  The status of every native call is asserted: the probe
bound's error flag is never raised."""
import ctypes

import numpy as np
import pytest

import barcode_census_expected as bx
import fragments_expected as fx
from rocco_amd import _native, dp, fragments as fr, tabix_index
from rocco_amd.bam import inflate_bgzf

pytestmark = pytest.mark.gpu
META, ARRAYS = bx.load_golden()
SHAPE = fr.barcode_census_shape()
ALLOWS = ("-", "empty", "nothing", "prefix", "some")
POISON = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    paths = bx.materialize(tmp_path_factory.mktemp("barcode_census"), META, ARRAYS)
    tabix_index.clear_tabix_index_cache()
    return paths


@pytest.fixture(scope="module")
def texts(files):
    return {key: bytes(inflate_bgzf(path)) for key, path in files.items() if not key.startswith("allow:")}


def allow_set(key):
    return set() if key == "-" else fx.parse_allowlist(bytes(ARRAYS[f"allow_{key}"]))


def source(files, key, allow="-"):
    return fr.FragmentsSource(files[key], None if allow == "-" else files["allow:" + allow])


def on_device(text):
    import torch

    return torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()


def same(got, twin, where):
    assert got.barcodes == twin.barcodes and np.array_equal(got.records, twin.records) and got.lines == twin.lines, where
    assert got.stats["status"] == _native.OK and got.stats["capacity"] >= 2 * len(got), where


def lines_text(barcodes):
    return b"".join(b"chr1\t%d\t%d\t%s\t1\n" % (i, i + 9, b) for i, b in enumerate(barcodes))


# ---- 1. every fixture file -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("slab_bytes", [fr.DEFAULT_SLAB_BYTES, 1])
@pytest.mark.parametrize("inflate", ["host", "device"])
def test_every_fixture_file_against_the_statement_the_twin_and_the_reference(gpu, files, texts, inflate, slab_bytes):
    """``slab_bytes=1``: every slab is one BGZF block (of about 2 500 bytes in "blocks"), so lines straddle slabs and the barcodes
    of the first slab return in the third and later ones: the compare against the arena."""
    stored = {(r["file"], r["allow"]): r for r in META["cells"]}
    for key in ("traps", "blocks", "ones", "nobarcode", "unindexed"):
        for allow in ALLOWS:
            got = fr.barcode_census(source(files, key, allow), inflate=inflate, slab_bytes=slab_bytes)
            bx.check(got, texts[key], allow_set(allow), (key, allow))
            same(got, fr.barcode_census_host(texts[key], source(files, key, allow).allowlist()), (key, allow))
            if "cells" in stored[(key, allow)]:
                assert len(got) == stored[(key, allow)]["cells"], (key, allow)
                if slab_bytes == 1:
                    assert fr.get_fragments_cell_count(source(files, key, allow), inflate=inflate, slab_bytes=1) == len(got)
            if slab_bytes == 1 and key == "blocks":
                assert got.stats["slabs"] >= len(META["files"]["blocks"]["cuts"]) > 8, got.stats
    with pytest.raises(RuntimeError, match="failed to load tabix index for fragments source"):
        fr.get_fragments_cell_count(files["unindexed"])
    cuts = META["files"]["blocks"]["cuts"]
    first, third = bx.census(texts["blocks"][: cuts[0]]), bx.census(texts["blocks"][texts["blocks"].rfind(b"\n", 0, cuts[1]) + 1: cuts[2]])
    assert set(first) & set(third) and texts["blocks"][cuts[0] - 1: cuts[0]] != b"\n"
    per_barcode = fr.barcode_census(files["ones"])
    assert dict(zip(per_barcode.barcodes, per_barcode.records.tolist())) == {r["barcode"].encode(): r["records"] for r in META["per_barcode"]}


# ---- 2. the structural edges ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["distinct", "equal"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, SHAPE["lines_per_turn"] - 1, SHAPE["lines_per_turn"] + 1,
                               SHAPE["max_grid"] * SHAPE["lines_per_turn"] + 1])
def test_line_counts_around_a_wavefront_a_turn_and_the_largest_grid(gpu, n, kind):
    """All barcodes distinct, and all equal: 64 lanes swap on one empty slot and one counter takes every add."""
    text = lines_text([b"BC%07d" % i for i in range(n)] if kind == "distinct" else [b"SAME-BARCODE-1"] * n)
    got = fr.barcode_census_device(on_device(text))
    same(got, fr.barcode_census_host(text), (n, kind))
    assert got.lines == n and len(got) == (n if kind == "distinct" else min(n, 1))
    if kind == "equal" and n:
        assert got.barcodes == [b"SAME-BARCODE-1"] and got.records.tolist() == [n]
    else:
        assert got.barcodes == [b"BC%07d" % i for i in range(n)] and np.array_equal(got.records, np.ones(n, dtype=np.int64))


def test_one_barcode_on_seventy_thousand_lines_is_counted_exactly(gpu):
    got = fr.barcode_census_device(on_device(lines_text([b"A"] * 70000)))
    assert got.barcodes == [b"A"] and got.records.tolist() == [70000] and got.lines == 70000 and got.stats["status"] == _native.OK


def mixed_text(seed, n_lines=4000, n_barcodes=300):
    rng = np.random.default_rng(seed)
    barcodes = [bytes(rng.integers(33, 256, size=int(rng.integers(1, 24))).astype(np.uint8)) for _ in range(n_barcodes)]
    barcodes += [barcodes[0] + b"x", barcodes[0][:-1] + b"\xfe" * 2, b"Z" * 300, b"Z" * 299 + b"Y"]
    picks = rng.integers(0, len(barcodes), size=n_lines)
    extra = [b"", b"\t", b"\t\t3", b"\r"]
    return b"".join(b"c\t%d\t%d" % (i, i + 5) + (b"\t" + barcodes[int(k)] + b"\t2" if i % 11 else extra[i % 4]) + b"\n" for i, k in enumerate(picks))


def test_the_result_does_not_depend_on_the_hash(gpu):
    """All ones, one bit and none: at mask 0 every lane starts at slot 0 and every decision is made by bytes alone along one
    probe chain."""
    text = mixed_text(7)
    want = fr.barcode_census_host(text)
    bx.check(want, text)
    assert 250 < len(want) <= 304
    for mask in (None, 1, 0):
        got = fr.barcode_census_device(on_device(text), hash_mask=mask)
        same(got, want, mask)
        same(fr.barcode_census_host(text, hash_mask=mask), want, mask)


def test_growing_from_the_smallest_table_over_several_slabs(gpu):
    import torch

    text = mixed_text(11, n_lines=6000)
    lines = text.split(b"\n")[:-1]
    want = fr.barcode_census_host(text)
    for mask in (None, 0):
        table = fr.BarcodeCensusTable(torch.device("cuda", torch.cuda.current_device()), hash_mask=mask, initial_capacity=SHAPE["min_capacity"])
        assert table.capacity == SHAPE["min_capacity"]
        at, capacities = 0, []
        for size in (10, 20, 50, 150, 400, 1500, 3870):
            part = on_device(b"".join(line + b"\n" for line in lines[at: at + size]))
            starts, _ = fr.lines_device(part)
            table.insert(part, starts)
            del part, starts  # (the slab is released: nothing of the table names it)
            capacities.append(table.capacity)
            at += size
        assert at == len(lines)
        got = table.census()
        assert got.stats["grows"] >= 3 and got.stats["slabs"] == 7 and capacities == sorted(capacities) and len(set(capacities)) >= 4, capacities
        same(got, want, mask)


def test_lines_without_a_barcode_give_an_empty_census(gpu, files):
    text = b"# only\nchrA\t1\t2\nchrA\t3\t4\t\t1\nchrA\t5\t6\t\n\n\r\nchrA\t7\t8\t\rBC\nchrA\t9\t10\t\x00BC"
    for got in (fr.barcode_census_device(on_device(text)), fr.barcode_census(files["nobarcode"]),
                fr.barcode_census_device(on_device(lines_text([b"AA", b"AB"])), allowlist=fr.parse_barcode_allowlist(b"A\nAAA\n"))):
        assert len(got) == 0 and got.barcodes == [] and got.records.shape == (0,) and got.packed[1].tolist() == [0]
        assert got.stats["status"] == _native.OK and got.stats["entries"] == 0
    assert fr.barcode_census_device(on_device(text)).lines == 8 and fr.get_fragments_cell_count(files["nobarcode"]) == 0


def test_two_runs_of_one_input_give_identical_arrays(gpu):
    text = mixed_text(3)
    runs = [fr.barcode_census_device(on_device(text)) for _ in range(2)]
    assert runs[0].barcodes == runs[1].barcodes and runs[0].records.tobytes() == runs[1].records.tobytes()
    assert runs[0].packed[0].tobytes() == runs[1].packed[0].tobytes() and runs[0].packed[1].tobytes() == runs[1].packed[1].tobytes()


# ---- 3. the C ABI with a guard element behind every array a kernel writes -------------------------------------------------

def guarded(n, dtype, fill=None):
    import torch

    t = torch.full((n + 1,), POISON if dtype == torch.int64 else 0x5A, dtype=dtype, device="cuda")
    if fill is not None:
        t[:n] = fill
    return t


def test_guard_elements_behind_every_output_array(gpu):
    import torch

    lib, solver = _native.load(), _native.solver_for(torch.cuda.current_device()).handle
    text = mixed_text(5, n_lines=1500, n_barcodes=90)
    want = fr.barcode_census_host(text)
    halves = [text[: text.index(b"\n", len(text) // 2) + 1], text[text.index(b"\n", len(text) // 2) + 1:]]
    capacity, entries, used = SHAPE["min_capacity"], 0, 0
    slots, counts = guarded(capacity, torch.int64, 0), guarded(capacity, torch.int64, 0)
    arena_bytes, arena_offsets, arena_hashes = guarded(0, torch.uint8), guarded(1, torch.int64, 0), guarded(1, torch.int64)
    stream = dp._stream_ptr(slots)
    report = (ctypes.c_longlong * 4)()
    for part in halves:
        data = on_device(part)
        starts, found = fr.lines_device(data)
        n_lines = found["lines"]
        # too small a table, too small an arena: refused before anything is launched
        assert lib.rocco_hip_barcode_census_insert(solver, data.data_ptr(), len(part), starts.data_ptr(), n_lines, None, None, 0, slots.data_ptr(),
                                                   counts.data_ptr(), capacity, arena_bytes.data_ptr(), 0, arena_offsets.data_ptr(),
                                                   arena_hashes.data_ptr(), 0, entries, used, fr.ALL_HASH_BITS, report, stream) == _native.EINVAL
        grown = capacity
        while grown < 2 * (entries + n_lines):
            grown *= 2
        new_slots, new_counts = guarded(grown, torch.int64), guarded(grown, torch.int64)
        assert lib.rocco_hip_barcode_census_rehash(solver, slots.data_ptr(), counts.data_ptr(), capacity, new_slots.data_ptr(), new_counts.data_ptr(),
                                                   grown, arena_hashes.data_ptr(), entries, fr.ALL_HASH_BITS, stream) == _native.OK
        slots, counts, capacity = new_slots, new_counts, grown
        more_bytes, more_offsets, more_hashes = guarded(used + len(part), torch.uint8), guarded(entries + n_lines + 1, torch.int64, 0), \
            guarded(entries + n_lines, torch.int64)
        more_bytes[:used], more_offsets[: entries + 1], more_hashes[:entries] = arena_bytes[:used], arena_offsets[: entries + 1], arena_hashes[:entries]
        arena_bytes, arena_offsets, arena_hashes = more_bytes, more_offsets, more_hashes
        assert lib.rocco_hip_barcode_census_insert(solver, data.data_ptr(), len(part), starts.data_ptr(), n_lines, None, None, 0, slots.data_ptr(),
                                                   counts.data_ptr(), capacity, arena_bytes.data_ptr(), used + len(part), arena_offsets.data_ptr(),
                                                   arena_hashes.data_ptr(), entries + n_lines, entries, used, fr.ALL_HASH_BITS, report,
                                                   stream) == _native.OK, _native.last_error()
        entries, used = entries + int(report[0]), used + int(report[1])
        for t in (slots, counts, arena_offsets, arena_hashes):
            assert int(t[-1]) == POISON
        assert int(arena_bytes[-1]) == 0x5A and int(arena_offsets[entries]) == used
    records = guarded(entries, torch.int64)
    assert lib.rocco_hip_barcode_census_records(solver, slots.data_ptr(), counts.data_ptr(), capacity, entries, records.data_ptr(), stream) == _native.OK
    assert int(records[-1]) == POISON and int((slots[:-1] != 0).sum()) == entries == len(want)
    got = fr.BarcodeCensus(arena_bytes[:used].cpu().numpy(), arena_offsets[: entries + 1].cpu().numpy(), records[:-1].cpu().numpy(), want.lines,
                           {"capacity": capacity, "grows": 2, "slabs": 2, "status": _native.OK})
    same(got, want, "guards")
    # a capacity that is no power of two, and a table too small for its entries, are refused
    assert lib.rocco_hip_barcode_census_records(solver, slots.data_ptr(), counts.data_ptr(), capacity - 1, entries, records.data_ptr(), stream) == _native.EINVAL
    assert lib.rocco_hip_barcode_census_rehash(solver, slots.data_ptr(), counts.data_ptr(), capacity, new_slots.data_ptr(), new_counts.data_ptr(),
                                               SHAPE["min_capacity"], arena_hashes.data_ptr(), entries, fr.ALL_HASH_BITS, stream) == _native.EINVAL
