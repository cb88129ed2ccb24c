"""The barcode census on the host (note (35)): the Python statement of ``ccounts_getCellCount``'s rule
(tests/barcode_census_expected.py, a dict over split lines) pinned to every stored answer of the reference, the host twin of the
kernels (`rocco_hip_barcode_census_host`) against that statement on every fixture at three hash masks, the allow-list round trip
and its refusals, the binding against the header, and the shared rules header under the host's sanitizers.  Nothing here
touches a device."""
import os
import subprocess

import numpy as np
import pytest

import barcode_census_expected as bx
import fragments_expected as fx
from rocco_amd import _native, fragments as fr
from rocco_amd.bam import inflate_bgzf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
META, ARRAYS = bx.load_golden()
MASKS = (None, 0x3, 0)
HAND = [b"", b"\n", b"\n\n", b"a", b"\t\t\tB", b"\t\t\tB\n", b"\t\t\t\n", b"\t\t\t", b"a\tb\tc\td\te\tf\n", b"a\tb\tc\tBC\rX\n", b"a\tb\r\tc\tBC\n",
        b"a\tb\tc\tB\x00C\n", b"\x00\t\t\tB\n", b"#a\tb\tc\tHASH\n#\n", b"a\tb\tc\tB\na\tb\tc\tB", b"a\tb\tc\tB\r\na\tb\tc\tBB\r\n", b"\r\n",
        b"a\tb\tc\t\xff\n" * 3 + b"a\tb\tc\t\xfe\n", b"a\tb\tc\t" + b"L" * 5000 + b"\n"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return bx.materialize(tmp_path_factory.mktemp("barcode_census"), META, ARRAYS)


@pytest.fixture(scope="module")
def texts(files):
    return {key: bytes(inflate_bgzf(path)) for key, path in files.items() if not key.startswith("allow:")}


def allow_set(key):
    return set() if key == "-" else fx.parse_allowlist(bytes(ARRAYS[f"allow_{key}"]))


def packed_list(files, key):
    return fr._NO_LIST if key == "-" else fr.load_barcode_allowlist(files["allow:" + key])


def test_the_statement_reproduces_every_stored_cell_count_and_per_barcode_count(texts):
    assert len(META["cells"]) >= 20 and len(META["per_barcode"]) == 12
    counted = 0
    for r in META["cells"]:
        if "error" in r:
            assert (r["file"], r["error"]) in (("unindexed", "failed to load tabix index for fragments source"),
                                               ("bam", "cell count is only supported for fragments sources")), r
            continue
        assert len(bx.census(texts[r["file"]], allow_set(r["allow"]))) == r["cells"], r
        assert texts[r["file"]].count(b"\n") + (not texts[r["file"]].endswith(b"\n")) == META["files"][r["file"]]["lines"]
        counted += 1
    assert counted >= 20 and {r["allow"] for r in META["cells"]} == {"-", "empty", "nothing", "prefix", "some"}
    ones = bx.census(texts["ones"])
    assert {r["barcode"].encode(): r["records"] for r in META["per_barcode"]} == ones and sum(ones.values()) == META["files"]["ones"]["lines"]
    # the fixtures hold what they were made for: an empty list file admits everything, a prefix of a barcode admits nothing of it
    by = {(r["file"], r["allow"]): r.get("cells") for r in META["cells"]}
    assert ARRAYS["allow_empty"].size == 0 and by[("traps", "empty")] == by[("traps", "-")] > 20 and by[("traps", "nothing")] == 0
    assert by[("traps", "prefix")] == 1 and by[("nobarcode", "-")] == 0 and not texts["traps"].endswith(b"\n")
    traps = bx.census(texts["traps"])
    assert {b"G", b"AC", b"ACG", b"ACGT", b"\x80", b"\xc3\xa9\xffB", b"META-FOUR-FIELDS", b"A B", b"#hash"} <= set(traps)
    assert sorted(len(b) for b in traps)[-2:] == [300, 300] and b"\x00" in texts["traps"] and b"AC\rGT" in texts["traps"]


@pytest.mark.parametrize("mask", MASKS)
def test_the_host_twin_equals_the_statement_on_every_fixture(files, texts, mask):
    for key, text in texts.items():
        for allow in ("-", "empty", "nothing", "prefix", "some"):
            got = fr.barcode_census_host(text, packed_list(files, allow), hash_mask=mask)
            bx.check(got, text, allow_set(allow), (key, allow, mask))
            assert got.stats["status"] == _native.OK and got.stats["capacity"] >= 2 * len(got)
    for text in HAND:
        bx.check(fr.barcode_census_host(text, hash_mask=mask), text, (), text[:40])
        bx.check(fr.barcode_census_host(text, fr.parse_barcode_allowlist(b"B\nBC\n\xff\n"), hash_mask=mask), text, {b"B", b"BC", b"\xff"}, text[:40])


def test_the_host_twin_grows_from_the_smallest_table_and_keeps_first_line_order():
    shape = fr.barcode_census_shape()
    assert shape["threads"] == shape["lines_per_turn"] == fr.fragfile_shape()["threads"] and shape["min_capacity"] & (shape["min_capacity"] - 1) == 0
    text = b"".join(b"c\t1\t2\tBC%05d\n" % (i % 700) for i in range(2000))
    for mask in MASKS:
        raw, offsets, records, lines, grows, capacity = fr.barcode_census_host_arrays(text, hash_mask=mask, initial_capacity=1)
        assert grows >= 3 and capacity >= 1400 and lines == 2000
        assert [bytes(raw[offsets[e]: offsets[e + 1]]) for e in range(700)] == [b"BC%05d" % i for i in range(700)]
        assert records.tolist() == [3 if i < 600 else 2 for i in range(700)]
    assert fr.barcode_census_host(text, initial_capacity=5000).stats == {"capacity": 8192, "grows": 0, "slabs": 1, "status": 0, "entries": 700}
    with pytest.raises(ValueError, match="hash_mask"):
        fr.barcode_census_host(text, hash_mask=-1)


def test_the_allowlist_round_trip_and_its_refusals(files, texts, tmp_path):
    census = fr.barcode_census_host(texts["ones"])
    for min_records in (1, int(np.median(census.records)) + 1, int(census.records.max()) + 1):
        path = tmp_path / f"list_{min_records}.txt"
        kept = [b for b, n in zip(census.barcodes, census.records) if n >= min_records]
        assert census.write_allowlist(path, min_records) == len(kept)
        assert path.read_bytes() == b"".join(b + b"\n" for b in kept)
        source = fr.FragmentsSource(files["ones"], str(path))
        packed, offsets = source.allowlist()
        assert [bytes(packed[offsets[i]: offsets[i + 1]]) for i in range(len(offsets) - 1)] == kept  # (census order is the loader's order)
        if kept:  # (an empty list admits everything, as the reference's does)
            again = fr.barcode_census_host(texts["ones"], source.allowlist())
            assert again.barcodes == kept and again.records.tolist() == [int(n) for n in census.records if n >= min_records]
    # bytes >= 0x80 and a barcode of 4 094 bytes go through; what the loader could not read back is refused by name
    edge = fr.barcode_census_host(b"c\t1\t2\t\xc3\xa9\xff\nc\t1\t2\t" + b"L" * 4094 + b"\n")
    edge.write_allowlist(tmp_path / "edge.txt")
    assert fr.load_barcode_allowlist(tmp_path / "edge.txt")[1].tolist() == list(edge.packed[1])
    for barcode, words in ((b"A B", "holds whitespace"), (b"#hash", "begins with `#`"), (b"L" * 4095, "has 4095 bytes"), (b"A\x0bB", "holds whitespace")):
        bad = fr.barcode_census_host(b"c\t1\t2\tGOOD\nc\t1\t2\t" + barcode + b"\nc\t1\t2\tGOOD\n")
        with pytest.raises(ValueError) as caught:
            bad.write_allowlist(tmp_path / "bad.txt")
        assert words in str(caught.value) and repr(barcode[:64])[2:-1] in str(caught.value) and not (tmp_path / "bad.txt").exists()
        assert bad.write_allowlist(tmp_path / "good.txt", min_records=2) == 1 and (tmp_path / "good.txt").read_bytes() == b"GOOD\n"
    with pytest.raises(ValueError, match="the barcode b'#hash' cannot stand in an allow-list"):  # (the first in census order)
        fr.barcode_census_host(texts["traps"]).write_allowlist(tmp_path / "traps.txt")


def test_the_header_declares_what_the_binding_binds():
    with open(os.path.join(ROOT, "include", "rocco_hip.h"), encoding="utf-8") as handle:
        header = handle.read()
    bound = {name for name, _, _ in _native.PROTOTYPES if name.startswith("rocco_hip_barcode_census_")}
    assert bound == {"rocco_hip_barcode_census_" + n for n in ("insert", "rehash", "records", "host", "shape")}
    for name, _, argtypes in _native.PROTOTYPES:
        if name in bound:
            declared = header[header.index(name + "("):]
            assert declared[: declared.index(";")].count(",") + 1 == len(argtypes), name
    shape = fr.barcode_census_shape()
    assert f"#define ROCCO_BARCODE_CENSUS_MAX_GRID {shape['max_grid']} " in header
    assert f"#define ROCCO_BARCODE_CENSUS_MIN_CAPACITY {shape['min_capacity']} " in header
    assert "ccounts_getCellCount (rocco/native/ccounts_backend.c:1890-2046)" in header
    assert "ccounts_getCellCount" not in fr.__doc__.split("Not read:")[1]


def test_the_entry_points_refuse_what_the_reference_refuses(files):
    with pytest.raises(RuntimeError, match="cell count is only supported for fragments sources"):
        fr.get_fragments_cell_count(os.path.join(os.path.dirname(files["ones"]), "reads.bam"))
    with pytest.raises(RuntimeError, match="failed to load tabix index for fragments source"):
        fr.get_fragments_cell_count(files["unindexed"])


# ---- the rules header under the sanitizers -------------------------------------------------------------------------------

def write_case(path, text, packed, mask, initial_capacity):
    raw, offsets, records, lines, _, _ = fr.barcode_census_host_arrays(text, packed, mask, initial_capacity)
    allow_bytes, allow_offsets = packed
    head = np.asarray([len(text), len(allow_offsets) - 1, int(allow_offsets[-1]), 0, initial_capacity, len(records), len(raw), lines], dtype=np.int64)
    head[3:4].view(np.uint64)[0] = fr.ALL_HASH_BITS if mask is None else mask
    with open(path, "wb") as handle:
        for part in (head, np.frombuffer(text, dtype=np.uint8), np.asarray(allow_offsets, dtype=np.int64), np.asarray(allow_bytes, dtype=np.uint8), raw,
                     offsets, records):
            handle.write(np.ascontiguousarray(part).tobytes())


def test_the_shared_rules_under_address_and_undefined_behaviour_sanitizers(files, texts, tmp_path):
    """tests/tools/barcode_census_san.cpp: the census functions of rocco_amd/csrc/fragments_rules.h -- what the kernels compile, and
    the host twin -- in one stand-alone executable built with -fsanitize=address,undefined, over `.case` files of every fixture
    text under every list and mask and of the hand-made edges, inputs and outputs in heap buffers of their exact size.  Exit
    code 0 and an empty sanitizer log (CPU only; nothing is loaded into Python, nothing is preloaded)."""
    case_dir = tmp_path / "cases"
    case_dir.mkdir()
    n = 0
    for key, text in texts.items():
        for allow in ("-", "nothing", "prefix", "some"):
            write_case(case_dir / f"{n:03d}.case", text, packed_list(files, allow), MASKS[n % 3], (1, 64, 1000)[n % 3])
            n += 1
    for text in HAND:
        for mask in MASKS:
            write_case(case_dir / f"{n:03d}.case", text, fr.parse_barcode_allowlist(b"B\nBC\n") if n % 2 else fr._NO_LIST, mask, 1)
            n += 1
    assert n >= 70
    program = str(tmp_path / "barcode_census_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-Wall", os.path.join(HERE, "tools", "barcode_census_san.cpp"), "-o", program], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([program] + sorted(str(p) for p in case_dir.glob("*.case")), capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"{n} files" in run.stdout and "all as expected" in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
