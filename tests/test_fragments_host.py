"""Fragments files on the host (note (34)): the Python statement of the reference's rules pinned
to every stored result of the reference's counter, the host twin of the kernels (`rocco_hip_fragfile_host`) against that
statement on every fixture file, the ``.tbi`` parser against the lines htslib's iterator yields, every refusal of the dialect
and of the container, the allow-list loader, the count-mode spellings, the read-length probe, and the shared rules header
under the host's sanitizers.  Nothing here touches a device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import fragments_expected as fx
from rocco_amd import _native, bam_index, fragments as fr, tabix_index
from rocco_amd.bam import inflate_bgzf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
META, ARRAYS = fx.load_golden()
MODES = fx.MODES


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    paths = fx.materialize(tmp_path_factory.mktemp("fragments"), META, ARRAYS)
    tabix_index.clear_tabix_index_cache()
    return paths


@pytest.fixture(scope="module")
def texts(files):
    return {key: bytes(inflate_bgzf(path)) for key, path in files.items() if not key.startswith("allow:")}


def allow_set(key):
    return set() if key == "-" else fx.parse_allowlist(bytes(ARRAYS[f"allow_{key}"]))


def contig_lines(text, contig):
    return [line for line in fx.split_lines(text) if line.startswith(b"#") or line.split(b"\t")[0] == contig.encode()]


# ---- the statement of the rules, pinned to the reference ----------------------------------------------------------------

def test_the_statement_reproduces_every_stored_count(texts):
    assert len(META["count"]) >= 100
    seen = set()
    for r in META["count"]:
        if "error" in r:
            assert r["error"] == "failed to open fragments region iterator" and r["contig"] == "chrNone"
            continue
        got = fx.count_region(contig_lines(texts[r["file"]], r["contig"]), allow_set(r["allow"]), r["start"], r["end"], r["step"], r["length"],
                              MODES[r["mode"]], r["one_read_per_bin"])
        assert got.tobytes() == ARRAYS[f"c_{r['name']}"].tobytes(), r["name"]
        seen.add((r["mode"], r["one_read_per_bin"], r["allow"] != "-"))
    assert len(seen) == 16  # every mode x one_read_per_bin x {no list, list}


def test_the_statement_reproduces_every_stored_range_mapped_count_and_read_length(texts):
    for r in META["range"]:
        kept = [line for line in contig_lines(texts[r["file"]], r["contig"]) if line.startswith(b"#") or int(line.split(b"\t")[1]) < r["chrom_len"]]
        assert fx.chrom_range(kept) == (r["start"], r["end"]), r
    for r in META["mapped"]:
        if "error" in r:
            assert r["file"] == "unindexed" and r["error"] == "failed to load tabix index for fragments source"
            continue
        got = fx.mapped_count(fx.split_lines(texts[r["file"]]), allow_set(r["allow"]), {e.encode() for e in r["exclude"]}, MODES[r["mode"]],
                              r["one_read_per_bin"])
        assert got == r["mapped"] and r["unmapped"] == 0, r
    for r in META["readlen"]:
        got = fx.read_length(fx.split_lines(texts[r["file"]]), r["min_reads"], r["max_iterations"])
        assert got == r.get("read_length"), r


def test_the_census_of_the_fixtures_names_every_rule():
    for rule in ("count:meta", "count:last_empty", "count:end_le_start", "count:barcode", "center:in", "center:outside", "center:beyond_buffer",
                 "cut:start:in", "cut:start:outside", "cut:end:in", "cut:end:outside", "coverage:in", "coverage:outside", "coverage:clipped",
                 "coverage:index0_beyond", "coverage:index1_clamped", "mapped:excluded", "mapped:short", "mapped:fifth_empty", "mapped:barcode",
                 "range:meta", "range:end_le_start", "range:in", "readlen:start", "readlen:end", "readlen:end_le_start", "readlen:in"):
        assert META["census"].get(rule, 0) > 0, rule


# ---- the container -------------------------------------------------------------------------------------------------------

def test_the_tabix_parser_finds_the_lines_htslibs_iterator_yields(files):
    """Per file and contig: the span `contig_span` names, inflated and split, without its meta lines, against the driver's dump --
    among them a contig that begins inside a block, one that begins on a block's first byte, one with a single line."""
    assert len(META["dump"]) >= 12
    for d in META["dump"]:
        want = bytes(ARRAYS[f"dump_{d['file']}_{d['contig']}"])
        span = fr.span_bytes_host(files[d["file"]], d["contig"])
        if d["contig"] == "chrNone":
            assert span is None and want == b""
            continue
        got = b"".join(line + b"\n" for line in fx.split_lines(span) if not line.startswith(b"#"))
        assert got == want, d
    index = tabix_index.open_tabix_index(files["blocks"])
    assert index.names == ["chrA", "chrB", "chrC"] and index.meta == ord("#") and index.tid_of["chrC"] == 2
    begin_b, begin_c = bam_index.contig_span(index, 1)[0], bam_index.contig_span(index, 2)[0]
    assert begin_b & 0xFFFF not in (0,) and tabix_index.open_tabix_index(files["blocks"]) is index  # (mid-block; the cache)
    assert fr.span_bytes_host(files["blocks"], "chrC").startswith(b"chrC\t") and begin_c > begin_b
    # chrB begins inside a block; chrC on a block's first byte (htslib names that place as the end of the block before it
    # or as the begin of the block itself), and the packer was told to end a block right there
    chr_b, chr_c = fr._stream_of(fr.FragmentsSource(files["blocks"]), "chrB", {}), fr._stream_of(fr.FragmentsSource(files["blocks"]), "chrC", {})
    assert 0 < chr_b.skip < chr_b.blocks[0][4] and chr_c.skip in (0, chr_c.blocks[0][4])
    text = bytes(inflate_bgzf(files["blocks"]))
    assert text.index(b"\nchrC\t") + 1 in META["files"]["blocks"]["cuts"] and text.index(b"\nchrB\t") + 1 not in META["files"]["blocks"]["cuts"]
    assert tabix_index.open_tabix_index(files["unindexed"]) is None


def tbi_bytes(n_ref=1, fmt=0x10000, cols=(1, 2, 3), meta=ord("#"), skip=0, names=b"chrA\x00", magic=b"TBI\x01", body=None):
    body = struct.pack("<i", 0) + struct.pack("<i", 0) if body is None else body  # (n_bin = 0, n_intv = 0)
    return magic + struct.pack("<8i", n_ref, fmt, cols[0], cols[1], cols[2], meta, skip, len(names)) + names + body * max(n_ref, 0)


@pytest.mark.parametrize("raw, words", [
    (tbi_bytes(magic=b"BAI\x01"), "magic b'BAI\\x01' where b'TBI\\x01' belongs (not a .tbi index)"),
    (tbi_bytes(fmt=2), "format of the header at file offset 8: it is 2 where the BED preset has 65536"),
    (tbi_bytes(fmt=0), "format of the header"),
    (tbi_bytes(cols=(1, 4, 5)), "col_beg of the header at file offset 16: it is 4 where the BED preset has 2"),
    (tbi_bytes(cols=(1, 2, 0)), "col_end of the header"),
    (tbi_bytes(cols=(2, 2, 3)), "col_seq of the header"),
    (tbi_bytes(skip=1), "skip of the header at file offset 28: it is 1 where the BED preset has 0"),
    (tbi_bytes(n_ref=-1), "n_ref is negative (-1)"),
    (tbi_bytes(n_ref=2), "they hold 1 names where n_ref says 2"),
    (tbi_bytes(names=b"chrA"), "the last name is not NUL-terminated"),
    (tbi_bytes()[:20], "the header at file offset 0: 36 bytes from there leave the file (20 bytes)"),
    (tbi_bytes()[:38], "the sequence names at file offset 36: 5 bytes from there leave the file (38 bytes)"),
    (tbi_bytes(body=struct.pack("<i", -3)), "n_bin of reference 0 at file offset 41: it is negative (-3)"),
    (tbi_bytes(body=struct.pack("<iIi", 1, 37450, 1) + bytes(16) + struct.pack("<i", 0)), "the pseudo-bin 37450 of reference 0"),
])
def test_every_refusal_of_the_container(raw, words):
    with pytest.raises(ValueError) as caught:
        tabix_index.parse_tabix_index(raw, "x.tbi")
    assert str(caught.value).startswith("x.tbi: ") and words in str(caught.value)


def test_a_sound_hand_built_index_parses_and_the_bai_parser_is_unchanged():
    chunk = struct.pack("<QQ", 5 << 16 | 3, 9 << 16)
    body = struct.pack("<iIi", 2, 4681, 1) + chunk + struct.pack("<Ii", 37450, 2) + chunk + struct.pack("<QQ", 7, 0) + struct.pack("<iQ", 1, 5 << 16)
    index = tabix_index.parse_tabix_index(tbi_bytes(body=body) + struct.pack("<Q", 0), "x.tbi")
    assert bam_index.contig_span(index, 0) == (5 << 16 | 3, 9 << 16) and bam_index.contig_stats(index, 0) == (7, 0) and index.n_no_coor == 0
    bai = bam_index.parse_bam_index(b"BAI\x01" + struct.pack("<i", 1) + body + struct.pack("<Q", 4), "x.bai")
    assert bai.bins[0].keys() == index.bins[0].keys() and bai.pseudo == index.pseudo and bai.n_intv == [1] and bai.n_no_coor == 4
    with pytest.raises(ValueError, match=r"x.bai: n_bin of reference 0 at file offset 8: it is negative \(-1\)"):
        bam_index.parse_bam_index(b"BAI\x01" + struct.pack("<ii", 1, -1), "x.bai")


# ---- the host twin against the statement ---------------------------------------------------------------------------------

def check_lines_against_statement(got, lines, allow, where):
    assert got["lines"] == len(lines), where
    for i, line in enumerate(lines):
        want, status = fx.status_word(line, allow), int(got["status"][i])
        assert bool(status & fr.META) == want["meta"], (where, i)
        if want["meta"]:
            assert status == fr.META
            continue
        assert (status >> fr.FIELDS_SHIFT) & fr.FIELDS_MASK == want["fields"], (where, i, line[:80])
        for bit, name in ((fr.START_OK, "start_ok"), (fr.END_OK, "end_ok"), (fr.LAST_EMPTY, "last_empty"), (fr.FIFTH_EMPTY, "fifth_empty"),
                          (fr.WEIGHT_PARSED, "weight_parsed"), (fr.BARCODE_PRESENT, "barcode_present"), (fr.BARCODE_ALLOWED, "barcode_allowed")):
            assert bool(status & bit) == want[name], (where, i, name, line[:80])
        assert status & (fr.NONCANONICAL | fr.BEYOND) == 0 or want["weight"] >= 2 ** 31
        assert (int(got["start"][i]), int(got["end"][i]), int(got["weight"][i])) == (want["start"], want["end"], want["weight"]), (where, i)


def test_the_host_twin_on_every_span_of_every_fixture_file(files):
    """Starts, fields and status words by equality with the statement; the counts the integer rule makes of them against the
    reference's stored counts, bit for bit wherever the magnitude stays within 2**24."""
    spans = {}
    for allow_key in ("-", "many", "one", "empty"):
        allow = allow_set(allow_key)
        packed = fr.load_barcode_allowlist(files["allow:" + allow_key]) if allow_key != "-" else fr._NO_LIST
        for key, info in META["files"].items():
            for contig in info["contigs"]:
                text = fr.span_bytes_host(files[key], contig)
                got = fr.fragfile_host(text, names=[contig], expect=[0], allowlists=[packed])
                assert got["report"] == (-1, 0), (key, contig)
                lines = fx.split_lines(text)
                offsets = np.concatenate([[0], np.cumsum([len(p) + 1 for p in text.split(b"\n")[:-1]])])[: len(lines)]
                assert np.array_equal(got["starts"][:-1], offsets) and got["starts"][-1] == len(text)
                assert got["open"] == (not text.endswith(b"\n")) and got["cut"] == text.rfind(b"\n") + 1
                check_lines_against_statement(got, lines, allow, (key, contig, allow_key))
                assert np.all(got["name"][(got["status"] & fr.META) == 0] == 0)
                spans[(key, contig, allow_key)] = got
    exact = refused = 0
    for r in META["count"]:
        if "error" in r:
            continue
        got = spans[(r["file"], r["contig"], r["allow"])]
        counts, magnitude = fx.counts_from_fields(got["start"], got["end"], got["weight"], got["status"], r["start"], r["end"], r["step"], r["length"],
                                                  MODES[r["mode"]], r["one_read_per_bin"])
        if magnitude <= 2 ** 24:
            assert counts.tobytes() == ARRAYS[f"c_{r['name']}"].tobytes(), r["name"]
            exact += 1
        else:
            refused += 1
    assert exact >= 100 and 1 <= refused <= 12


def test_the_host_twin_on_whole_files_and_the_read_length_probe(files, texts):
    for key in ("mixed", "blocks", "plain", "unindexed"):
        got = fr.fragfile_host(texts[key], whole_file=True, names=["chrB", "chrX"], allowlists=[fr.load_barcode_allowlist(files["allow:many"])])
        assert got["report"] == (-1, 0)
        lines, allow = fx.split_lines(texts[key]), allow_set("many")
        ok = (got["name"] < 0) & ((got["status"] & fr.FIFTH_EMPTY) == 0) & ((got["status"] & fr.BARCODE_ALLOWED) != 0)
        assert int(got["weight"][ok].astype(np.int64).sum()) == fx.mapped_count(lines, allow, {b"chrB", b"chrX"}, 0, 0)
    for r in META["readlen"]:
        if "error" in r:
            with pytest.raises(RuntimeError, match="failed to estimate fragment length from fragments source"):
                fr.get_fragments_read_length(files[r["file"]], r["min_reads"], r["max_iterations"])
        else:
            assert fr.get_fragments_read_length(files[r["file"]], r["min_reads"], r["max_iterations"]) == r["read_length"], r


# ---- the dialect ---------------------------------------------------------------------------------------------------------

SOUND = b"chrA\t10\t20\tAA\t1\n"
DIALECT = [
    (b"chrA\t30\n", fr.ERR_FIELDS), (b"chrA\n", fr.ERR_FIELDS), (b"\n", fr.ERR_FIELDS), (b"chrA\t30\t\n", fr.ERR_FIELDS),
    (b"chrA\t010\t40\n", fr.ERR_NONCANONICAL), (b"chrA\t0x1f\t40\n", fr.ERR_NONCANONICAL), (b"chrA\t+30\t40\n", fr.ERR_NONCANONICAL),
    (b"chrA\t 30\t40\n", fr.ERR_NONCANONICAL), (b"chrA\t30abc\t40\n", fr.ERR_NONCANONICAL), (b"chrA\t-3\t40\n", fr.ERR_NONCANONICAL),
    (b"chrA\t30\t4e1\n", fr.ERR_NONCANONICAL), (b"chrA\t\t40\n", fr.ERR_NONCANONICAL), (b"chrA\t30\t2147483648\n", fr.ERR_BEYOND),
    (b"chrA\t2147483648\t2147483649\n", fr.ERR_BEYOND), (b"chrA\t30\t99999999999999999999999\n", fr.ERR_BEYOND),
    (b"chrA\t30\t40\tA\x00A\t1\n", fr.ERR_NUL), (b"chrA\t30\t40\tA\rA\t1\n", fr.ERR_CR), (b"chrA\t30\t40\r\r\n", fr.ERR_CR),
    (b"chrB\t30\t40\n", fr.ERR_CONTIG), (b"chrAA\t30\t40\n", fr.ERR_CONTIG), (b"chr\t30\t40\n", fr.ERR_CONTIG), (b"chrA\t9\t40\n", fr.ERR_ORDER),
    (b"chrA\t30\t40\tAA\t1234567890123456789\n", fr.ERR_COUNT), (b"chrA\t30\t40\tAA\t2147483648\n", fr.ERR_COUNT),
    (b"chrA\t30\t40\tAA\t-1234567890123456789\n", fr.ERR_COUNT),
]
ACCEPTED = [b"chrA\t30\t40\tAA\t2147483647\n", b"chrA\t30\t40\tAA\t123456789012345678x\n", b"chrA\t10\t2147483647\n", b"chrA\t30\t40\tAA\t-5\n",
            b"chrA\t30\t30\n", b"chrA\t30\t20\n", b"# chrB\t1\n", b"#\n", b"chrA\t30\t40\r\n", b"chrA\t30\t40\t\t\t\t\t\t\n", b"chrA\t10\t11\n"]


@pytest.mark.parametrize("line, code", DIALECT)
def test_every_refusal_of_the_dialect(line, code):
    """One hand-built span per rule: the offending line between two sound ones is the first the report names, with its code;
    alone and unterminated it is named as well."""
    got = fr.fragfile_host(SOUND + line + b"chrA\t50\t60\n", names=["chrA"], expect=[0])
    assert got["report"] == (1, code)
    if line != b"\n" and code != fr.ERR_ORDER:
        assert fr.fragfile_host(line[:-1], names=["chrA"], expect=[0])["report"] == (0, code)
    assert code in fr._ERROR_TEXT and fr._ERROR_TEXT[code]


def test_the_lowest_code_of_the_first_offending_line_is_reported():
    got = fr.fragfile_host(SOUND + b"chrA\t50\t60\n" + b"chrB\t07\t40\tA\x00\t1\n" + b"chrA\t1\n", names=["chrA"], expect=[0])
    assert got["report"] == (2, fr.ERR_NUL)
    got = fr.fragfile_host(SOUND + b"chrB\t7\t40\n", names=["chrA"], expect=[0])
    assert got["report"] == (1, fr.ERR_CONTIG)  # (and out of order: the contig rule has the lower code)
    got = fr.fragfile_host(SOUND + b"chrB\t7\t40\n", names=["chrA"], expect=[-1])
    assert got["report"] == (1, fr.ERR_ORDER)


@pytest.mark.parametrize("line", ACCEPTED)
def test_what_the_dialect_accepts(line):
    assert fr.fragfile_host(SOUND + line + b"chrA\t50\t60\n", names=["chrA"], expect=[0])["report"] == (-1, 0)


def test_whole_file_lines_read_meta_and_short_lines_as_the_reference_does():
    text = b"#chrA\tx\t-4\tAA\t3\nchrA\nchrA\t5\n\nchrA\t7\t9\tAA\nchrA\t7\t9\tAA\t\nchrA\t9\t8\tAA\t2\n#c\t-3\t5\n"
    got = fr.fragfile_host(text, whole_file=True)
    assert got["report"] == (-1, 0) and got["lines"] == 8
    assert [bool(s & fr.FIFTH_EMPTY) for s in got["status"]] == [False, True, True, True, True, True, False, True]
    assert (int(got["start"][7]), int(got["end"][7])) == (-3, 5) and got["status"][7] & fr.START_OK and not got["status"][0] & fr.START_OK
    assert fr.fragfile_host(b"chrA\t07\t9\n", whole_file=True)["report"] == (0, fr.ERR_NONCANONICAL)
    assert fr.fragfile_host(b"chrA\t7\t9\tAA\t99999999999\n", whole_file=True)["report"] == (0, fr.ERR_COUNT)
    two = fr.fragfile_host(SOUND + b"chrB\t1\t2\n" + SOUND, track_first=[0, 2, 3], expect=[-1, 0], names=["chrA"],
                           allowlists=[fr._NO_LIST, fr.parse_barcode_allowlist(b"AB\n")])
    assert two["report"] == (1, fr.ERR_ORDER) and not two["status"][2] & fr.BARCODE_ALLOWED and two["status"][0] & fr.BARCODE_ALLOWED


# ---- allow-lists, modes, the header --------------------------------------------------------------------------------------

def test_the_allowlist_loader_follows_the_references_rules(files, tmp_path):
    for key in META["allowlists"]:
        packed, offsets = fr.load_barcode_allowlist(files["allow:" + key])
        entries = [bytes(packed[offsets[i]: offsets[i + 1]]) for i in range(len(offsets) - 1)]
        assert entries == sorted(fx.parse_allowlist(bytes(ARRAYS[f"allow_{key}"]))) and len(entries) == META["allowlists"][key]["entries"]
    assert META["allowlists"]["empty"]["entries"] == 0 and META["allowlists"]["one"]["entries"] == 1 and META["allowlists"]["many"]["entries"] >= 300
    packed, offsets = fr.parse_barcode_allowlist(b"  B x\n#C\n\n\tA\r\nB\nAB\n \n")
    assert bytes(packed) == b"AABB" and offsets.tolist() == [0, 1, 3, 4]
    fr.parse_barcode_allowlist(b"A" * 4094 + b"\n")
    fr.parse_barcode_allowlist(b"A\n" + b"C" * 4095)  # (an unterminated last line of 4 095 bytes fits fgets' buffer whole)
    with pytest.raises(ValueError, match="line 2 of the barcode allow-list has 4096 bytes"):
        fr.parse_barcode_allowlist(b"A\n" + b"C" * 4096)
    changing = tmp_path / "changing.txt"
    changing.write_bytes(b"AA\n")
    src = fr.FragmentsSource(files["plain"], str(changing))
    assert src.allowlist()[1].tolist() == [0, 2]
    changing.write_bytes(b"AA\nCCC\n")
    assert src.allowlist()[1].tolist() == [0, 2, 5]  # (the list follows the file, as the key of the cached lines does)
    with pytest.raises(ValueError, match="line 2 of the barcode allow-list has 4096 bytes"):
        fr.parse_barcode_allowlist(b"A\n" + b"C" * 4095 + b"\n", "list.txt")
    with pytest.raises(ValueError, match="holds a NUL byte"):
        fr.parse_barcode_allowlist(b"A\x00\n")
    with pytest.raises(RuntimeError, match="failed to open barcode allowlist"):
        fr.FragmentsSource(files["plain"], str(tmp_path / "missing.txt")).allowlist()


def test_the_count_mode_spellings():
    for names, mode in ((("coverage", "cov", "0"), 0), (("cutsite", "cut", "cutsites", "1"), 1), (("fiveprime", "five_prime", "5p", "2"), 2),
                        (("center", "centre", "midpoint", "3"), 3)):
        assert all(fr.parse_count_mode(name) == mode for name in names)
    for bad in ("Coverage", "", "4", "cuts", None, 1):
        with pytest.raises(ValueError, match="unsupported count mode"):
            fr.parse_count_mode(bad)


def test_the_header_declares_what_the_binding_binds():
    with open(os.path.join(ROOT, "include", "rocco_hip.h"), encoding="utf-8") as handle:
        header = handle.read()
    bound = {name for name, _, _ in _native.PROTOTYPES if name.startswith("rocco_hip_fragfile_")}
    assert bound == {"rocco_hip_fragfile_" + n for n in ("lines", "fields", "count_batch", "chrom_range_batch", "mapped_count", "host", "shape")}
    for name, _, argtypes in _native.PROTOTYPES:
        if name in bound:
            declared = header[header.index(name + "("):]
            assert declared[: declared.index(";")].count(",") + 1 == len(argtypes), name
    for name in ("META", "START_OK", "END_OK", "LAST_EMPTY", "FIFTH_EMPTY", "WEIGHT_PARSED", "BARCODE_PRESENT", "BARCODE_ALLOWED", "NONCANONICAL",
                 "BEYOND"):
        assert f"#define ROCCO_FRAGFILE_{name} 0x{getattr(fr, name):x}u" in header
    for name in ("FIELDS", "NUL", "CR", "NONCANONICAL", "BEYOND", "COUNT", "CONTIG", "ORDER"):
        assert f"#define ROCCO_FRAGFILE_ERR_{name} {getattr(fr, 'ERR_' + name)}\n" in header
    shape = fr.fragfile_shape()
    assert shape["tile_bytes"] == 16 * shape["threads"] and shape["lines_per_turn"] == shape["threads"]
    assert "stay\n * outside" not in header and "row f13 (rocco_hip_fragfile_* below)" in header


# ---- the rules header under the sanitizers -------------------------------------------------------------------------------

def write_case(path, text, whole_file, names, expect, packed, entry0=0):
    got = fr.fragfile_host(text, entry0=entry0, whole_file=whole_file, names=names, expect=[expect], allowlists=[packed])
    name_bytes = b"".join(n.encode() for n in names)
    name_offsets = np.concatenate([[0], np.cumsum([len(n) for n in names])]).astype(np.int64)
    allow_bytes, allow_offsets = packed
    head = np.asarray([len(text), entry0, int(whole_file), len(names), len(name_bytes), len(allow_offsets) - 1, int(allow_offsets[-1]), expect,
                       got["lines"], got["cut"], int(got["open"]), got["report"][0], got["report"][1]], dtype=np.int64)
    with open(path, "wb") as handle:
        for part in (head, np.frombuffer(text, dtype=np.uint8), name_offsets, np.frombuffer(name_bytes, dtype=np.uint8),
                     np.asarray(allow_offsets, dtype=np.int64), np.asarray(allow_bytes, dtype=np.uint8), got["starts"], got["start"], got["end"],
                     got["weight"], got["name"], got["status"]):
            handle.write(np.ascontiguousarray(part).tobytes())


def test_the_shared_rules_under_address_and_undefined_behaviour_sanitizers(files, texts, tmp_path):
    """tests/tools/fragments_rules_san.cpp: rocco_amd/csrc/fragments_rules.h -- the functions the kernels compile -- in one
    stand-alone executable built with -fsanitize=address,undefined, over `.case` files of every span and whole file of the
    fixtures, every refusal and every accepted edge (each also without its last byte), with inputs and outputs allocated at
    their exact sizes.  Exit code 0 and an empty sanitizer log (CPU only; nothing is loaded into Python, nothing is preloaded)."""
    case_dir = tmp_path / "cases"
    case_dir.mkdir()
    many, n = fr.load_barcode_allowlist(files["allow:many"]), 0
    for key, info in META["files"].items():
        for contig in info["contigs"]:
            write_case(case_dir / f"{n:03d}.case", fr.span_bytes_host(files[key], contig), False, [contig], 0, many if n % 2 else fr._NO_LIST)
            n += 1
    for key in ("mixed", "blocks", "unindexed", "header_only"):
        write_case(case_dir / f"{n:03d}.case", texts[key], True, ["chrB", "chrX"], -1, many)
        write_case(case_dir / f"{n + 1:03d}.case", texts[key], True, [], -1, fr._NO_LIST, entry0=min(7, len(texts[key])))
        n += 2
    for line in [d[0] for d in DIALECT] + ACCEPTED + [b"", b"\n", b"\n\n", b"a", b"\t", b"\t\t\t\t\t\t"]:
        for text in (SOUND + line + b"chrA\t50\t60\n", line, line[:-1]):
            write_case(case_dir / f"{n:03d}.case", text, False, ["chrA"], 0, many)
            n += 1
    assert n >= 120
    program = str(tmp_path / "fragments_rules_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-Wall", os.path.join(HERE, "tools", "fragments_rules_san.cpp"), "-o", program], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([program] + sorted(str(p) for p in case_dir.glob("*.case")), capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"{n} files" in run.stdout and "all as expected" in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
