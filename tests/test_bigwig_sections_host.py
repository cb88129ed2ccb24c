"""The section decode of bigWig files on the CPU (note (31)): `rocco_hip_bigwig_sections_host`, the host twin that
compiles the kernels' rules (rocco_amd/csrc/bigwig_sections.h), against the second reader of tests/bigwig_files.py on every file of
`valid_cases()` and of bigwig_score_cases.py, by bit pattern; one hand-built section per refusal; the refusals of the entry point itself;
and the same functions over the same cases as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bigwig_files as bf
import bigwig_sections_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return cases.file_inputs(cases.write_all(tmp_path_factory.mktemp("bigwig_sections")))


def decode(sections, tid, length, **how):
    from rocco_amd import bigwig

    slots, table, produced = cases.layout(sections, **how)
    return bigwig.decode_sections_host(slots, table, produced, [0, len(sections)], [tid], [length])


def same(got, expected):
    starts, ends, bits = expected
    return np.array_equal(got["starts"], starts) and np.array_equal(got["ends"], ends) and \
        np.array_equal(got["values"].view(np.uint64), cases.widened_bits(bits))


def test_the_cases_make_the_decode_do_what_they_claim(inputs):
    seen = cases.census(inputs)
    assert seen["types"] == {1, 2, 3}
    assert seen["skipped"] >= 1 and seen["dropped_at_end"] >= 3 and seen["all_dropped"] >= 1 and seen["trailing"] >= 1
    assert {1, 63, 64, 65, 1024} <= seen["counts"]
    assert sum(len(sections) == 0 for _, sections, _, _, _ in inputs) >= 1  # (a chromosome with no section)
    assert sum(len(sections) > 256 for _, sections, _, _, _ in inputs) >= 1


def test_host_twin_against_the_second_reader_on_every_file(inputs):
    for label, sections, tid, length, expected in inputs:
        got = decode(sections, tid, length)
        assert got["report"]["block"] == -1 and not got["status"].any(), label
        assert same(got, expected), label
        assert got["file_offsets"].tolist() == [0, expected[0].size] and got["report"]["produced"] == expected[0].size, label
        assert got["block_first"][0] == 0 and np.all(np.diff(got["block_first"]) >= 0) and got["block_first"][-1] == expected[0].size, label


def test_host_twin_against_the_writers_input(tmp_path):
    """`intervals_of_sections` reads no file: the same rules over what the writer was given."""
    for index, (label, chroms, sections, how, asked) in enumerate(bf.valid_cases()):
        path, record = bf.write_case((label, chroms, sections, how, asked), tmp_path, index)
        for chromosome in asked:
            if chromosome in record["chroms"]:
                tid, length = record["chroms"][chromosome]
                got = decode(cases.file_sections(path, record, chromosome), tid, length)
                assert same(got, bf.as_arrays(bf.intervals_of_sections(sections, tid, length))), (label, chromosome)


def test_several_files_in_one_table(inputs):
    from rocco_amd import bigwig

    chosen = [entry for entry in inputs if len(entry[1]) <= 8][:24]
    assert len(chosen) >= 20 and any(len(entry[1]) == 0 for entry in chosen)
    sections = [s for entry in chosen for s in entry[1]]
    slots, table, produced = cases.layout(sections)
    first = np.cumsum([0] + [len(entry[1]) for entry in chosen])
    got = bigwig.decode_sections_host(slots, table, produced, first, [e[2] for e in chosen], [e[3] for e in chosen])
    assert got["report"]["block"] == -1
    for k, (label, _, _, _, expected) in enumerate(chosen):
        lo, hi = got["file_offsets"][k], got["file_offsets"][k + 1]
        view = {name: got[name][lo:hi] for name in ("starts", "ends", "values")}
        assert same(view, expected), label


@pytest.mark.parametrize("label, data, want", cases.refusals(), ids=[r[0] for r in cases.refusals()])
def test_one_section_per_refusal(label, data, want):
    good = bf.section_bytes(bf.fixed_sections(0, 1, 3, seed=1)[0])
    alone = decode([data], 0, 10 ** 7, capacity=len(data))
    assert alone["status"].tolist() == [want] and alone["report"] == {"block": 0, "status": want, "produced": 0} and alone["starts"] is None
    among = decode([good, data, good, data], 0, 10 ** 7)
    assert among["status"].tolist() == [0, want, 0, want] and among["report"]["block"] == 1 and among["report"]["status"] == want
    assert among["block_first"].tolist() == [0, 3, 3, 6, 6] and among["starts"] is None  # (a refused block keeps nothing)


@pytest.mark.parametrize("label, data, length, want", cases.accepted_edges(), ids=[r[0] for r in cases.accepted_edges()])
def test_sections_at_the_edge_of_a_rule(label, data, length, want):
    got = decode([data], 0, length)
    assert got["status"].tolist() == [0] and got["report"]["block"] == -1
    if want is not None:
        assert same(got, bf.as_arrays(want))
    else:  # the four bit patterns: what C's (double) makes of them on x86-64
        assert got["values"].view(np.uint64).tolist() == [0x7FF82468A0000000, 0xFFF8000020000000, 0x8000000000000000, 0x36B8000000000000]
        assert np.array_equal(got["values"].view(np.uint64), cases.widened_bits(np.frombuffer(data[24:], dtype=np.uint32)))


def test_the_poisoned_tail_of_a_slot_is_never_read():
    """The same sections with other bytes behind `produced`, inside the slot's capacity: the same result."""
    sections = [bf.section_bytes(s) for s in bf.fixed_sections(0, 3, 5, seed=2) + bf.bed_sections(0, 1, 2, first=2000, seed=3)]
    a = decode(sections, 0, 10 ** 7, capacity=4096)
    b = decode(sections, 0, 10 ** 7, capacity=4096, poison=False)
    assert a["starts"].size == 17 and all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in ("starts", "ends", "values"))


def test_what_the_entry_point_refuses():
    from rocco_amd import _native, bigwig

    sections = [bf.section_bytes(s) for s in bf.fixed_sections(0, 2, 5, seed=4)]
    slots, table, produced = cases.layout(sections)
    one = ([0, 2], [0], [10 ** 7])
    for column, value in ((3, slots.size - 10), (3, -8), (2, -1), (2, slots.size + 1)):  # a row outside the slots
        bad = table.copy()
        bad[1, column] = value
        got = bigwig.decode_sections_host(slots, bad, produced, *one)
        assert got["status"].tolist() == [0, cases.ERR_TABLE] and got["report"]["block"] == 1 and got["block_first"].tolist() == [0, 5, 5]
    for value in (int(table[0, 2]) + 1, -1):  # produced > capacity
        got = bigwig.decode_sections_host(slots, table, np.asarray([value, produced[1]]), *one)
        assert got["status"].tolist() == [cases.ERR_TABLE, 0] and got["report"] == {"block": 0, "status": cases.ERR_TABLE, "produced": 5}
    for first in ([0, 1], [1, 2], [0, 3], [0, 2, 1, 2]):  # file offsets that do not ascend from 0 to n
        with pytest.raises(ValueError, match="rocco_hip_bigwig_sections_host"):
            bigwig.decode_sections_host(slots, table, produced, first, [0] * (len(first) - 1), [10 ** 7] * (len(first) - 1))
    # the C entry point itself: an output smaller than the total, a null pointer with a size, outputs given in part
    lib, ll = _native.load(), bigwig._ll
    first, ids, lengths = bigwig._file_arrays(*one)
    status, block_first, offsets = np.zeros(2, dtype=np.int32), np.zeros(3, dtype=np.int64), np.zeros(2, dtype=np.int64)
    out = [np.full(10 + 64, -7, dtype=np.int64), np.full(10 + 64, -7, dtype=np.int64), np.full(10 + 64, -7.0, dtype=np.float64)]

    def call(sizes=(10, 10, 10), pointers=(True, True, True), n_status=2, n_first=3, slots_ptr=slots.ctypes.data):
        back = (ctypes.c_longlong * 4)()
        args = [a.ctypes.data if given else None for a, given in zip(out, pointers)]
        return lib.rocco_hip_bigwig_sections_host(None, slots_ptr, slots.size, table.ctypes.data, produced.ctypes.data, 2, ll(first), ll(ids),
                                                  ll(lengths), 1, status.ctypes.data, n_status, block_first.ctypes.data, n_first, ll(offsets),
                                                  args[0], sizes[0], args[1], sizes[1], args[2], sizes[2], back)

    assert call() == _native.OK and out[0][:10].tolist() == [50 * j for j in range(10)] and all(np.all(a[10:] == -7) for a in out)
    for a in out:
        a[:] = -7
    for sizes in ((9, 10, 10), (10, 9, 10), (10, 10, 9), (0, 0, 0)):
        assert call(sizes=sizes) == _native.EINVAL, sizes
    for pointers in ((False, True, True), (True, False, True), (True, True, False)):
        assert call(pointers=pointers) == _native.EINVAL, pointers
    assert call(n_status=1) == _native.EINVAL and call(n_first=2) == _native.EINVAL and call(slots_ptr=None) == _native.EINVAL
    assert all(np.all(a == -7) for a in out)  # (a refused call writes nothing)
    assert call(sizes=(0, 0, 0), pointers=(False, False, False)) == _native.OK  # (the first stage alone)


def test_shape_and_constants():
    from rocco_amd import bigwig

    assert bigwig.sections_shape() == {"threads": 64, "max_grid": 1 << 16, "header_bytes": 24}
    assert (bigwig.BIGWIG_ERR_SHORT, bigwig.BIGWIG_ERR_TYPE, bigwig.BIGWIG_ERR_ITEMS, bigwig.BIGWIG_ERR_WRAP) == \
        (cases.ERR_SHORT, cases.ERR_TYPE, cases.ERR_ITEMS, cases.ERR_WRAP)
    header = open(os.path.join(os.path.dirname(HERE), "include", "rocco_hip.h"), encoding="utf-8").read()
    for name, value in (("SHORT", 8), ("TYPE", 9), ("ITEMS", 10), ("WRAP", 11)):
        assert f"#define ROCCO_BIGWIG_ERR_{name} {value}\n" in header


def test_the_shared_rules_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/tools/bigwig_sections_san.cpp: rocco_amd/csrc/bigwig_sections.h -- the functions the kernels compile -- in one
    stand-alone executable built with -fsanitize=address,undefined, over the `.case` files of every input above (the files of both
    case lists, every refusal alone in a buffer of exactly its bytes and between sound sections, the accepted edges), with
    slots and outputs allocated at their exact sizes.  Exit code 0 and an empty sanitizer log (CPU only; nothing is loaded
    into Python, nothing is preloaded)."""
    case_dir = tmp_path / "cases"
    case_dir.mkdir()
    n = cases.write_case_files(case_dir, tmp_path)
    assert n >= 60
    program = str(tmp_path / "bigwig_sections_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-Wall", os.path.join(HERE, "tools", "bigwig_sections_san.cpp"), "-o", program], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([program] + sorted(str(p) for p in case_dir.glob("*.case")), capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"{n} files" in run.stdout and "all as expected" in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
