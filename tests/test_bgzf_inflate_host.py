"""CPU: the decode rules of csrc/inflate_core.h through their host entry (rocco_hip_bgzf_inflate_host: the source the kernels of
csrc/bgzf_inflate.hip are compiled from, on one thread over host memory) against the host path's zlib on every case of
tests/bgzf_expected.py -- bytes equal or refused by the same check, block by block -- and the helper's own claims."""
import os
import re
import zlib

import numpy as np
import pytest

import bgzf_expected as gx


def run_host(raw: bytes, label: str = "") -> int:
    """The host entry over a whole file into a guarded buffer, verified; the first refused block or -1."""
    from rocco_amd import bam

    table, n_out = gx.guarded_table(raw)
    out = np.full(n_out, gx.GUARD_BYTE, dtype=np.uint8)
    status, report = bam.inflate_blocks_host(raw, table, out)
    first = gx.verify(raw, table, status, out, label)
    assert report["block"] == first and report["status"] == (int(status[first]) if first >= 0 else 0), label
    if first >= 0 and report["status"] == gx.ERR_LENGTH:
        _, lo, hi, _, _ = gx.blocks_of(raw)[first]
        assert report["produced"] == len(zlib.decompress(raw[lo:hi], wbits=-15)), label
    return first


def test_the_helpers_own_claims():
    """What the case lists say of themselves, checked with zlib and the existing host path."""
    from rocco_amd import bam

    for label, cdata, data in gx.hand_streams() + gx.census_streams():
        assert zlib.decompress(cdata, wbits=-15) == data, label
        assert gx.scan(cdata)[1] == len(data), label  # (the census walks the stream as zlib does)
    sizes = {label.split(":")[0]: (len(cdata), len(data)) for label, cdata, data in gx.census_streams()[1:]}
    assert gx.census_streams()[0][0].startswith("long codes") and len(gx.census_streams()[0][2]) > 32768 + 3 * 258
    assert sizes["the largest stored block"] == (gx.MAX_STORED + 5, gx.MAX_STORED) and gx.MAX_STORED == 65505
    assert len(gx.around(b"\0" * (gx.MAX_STORED + 5), b"")) == 0x10000  # (one byte more and `block` refuses it)
    assert gx.stage_bytes() == 512 and len(gx.stage_edges()) == 20
    stored = gx.deflate(gx.random_bytes(65280, 1), level=0)
    # several stored blocks in one BGZF block, 5 bytes of header each, the first not final: 65 290 bytes where zlib writes the
    # payload whole and closes with an empty block, 65 316 where it cuts the payload first
    assert stored[0] & 7 == 0 and len(stored) in (65290, 65316) and zlib.decompress(stored, wbits=-15) == gx.random_bytes(65280, 1)
    assert len(gx.deflate(bytes(65536), strategy=zlib.Z_RLE)) < 128  # (79 with zlib 1.2.11: distance-1 copies of 258)
    for name in ("Z_FULL_FLUSH", "Z_SYNC_FLUSH"):
        flushed = gx.deflate(gx.text_bytes(3000, 2), flushes=(1000, 2000), flush_mode=getattr(zlib, name))
        assert flushed.count(b"\x00\x00\xff\xff") >= 2 and zlib.decompress(flushed, wbits=-15) == gx.text_bytes(3000, 2)
    labels = [label for label, _ in gx.valid_files()]
    assert len(set(labels)) == len(labels) >= 55
    for label, raw in gx.valid_files():
        want = gx.outcomes(raw)
        assert all(code == 0 for code, _ in want), label
        assert bam.inflate_bgzf(raw).tobytes() == b"".join(data for _, data in want), label
    assert sorted(len(gx.blocks_of(raw)) for label, raw in gx.valid_files() if "blocks, end-of-file marker in" in label) == [2, 3, 65, 66, 601]
    text = gx.deflate(gx.text_bytes(65280, 2))
    assert text[0] & 6 == 4  # a dynamic block


def test_every_corrupt_case_is_refused_by_the_host_path():
    from rocco_amd import bam

    cases = gx.corrupt_files()
    assert len({label for label, *_ in cases}) == len(cases) >= 45
    for label, raw, index, code in cases:
        want = gx.outcomes(raw)
        assert want[index][0] == code and all(c == 0 for c, _ in want[:index]), label
        with pytest.raises(ValueError, match=gx.error_pattern(raw, index, code)):
            bam.inflate_bgzf(raw)


def test_the_valid_files_make_a_decoder_do_everything():
    """The census of `valid_files()` (every distinct deflate span scanned once): what the valid cases, together, decode.  Every
    stream of `census_streams()` is needed for it: without the first long-code stream "a distance code length is never decoded"
    fires, without the code-length-code stream "no code-length code holds all seven lengths at once", and so on for each."""
    spans = {bytes(raw[lo:hi]) for _, raw in gx.valid_files() for _, lo, hi, _, _ in gx.blocks_of(raw)}
    seen = gx.census(spans)
    assert seen["lit_bits"] == set(range(1, 16)), "a literal/length code length is never decoded"
    assert seen["dist_bits"] == set(range(1, 16)), "a distance code length is never decoded"
    both = lambda n: {(s, ends) for s in range(n) for ends in ("zeros", "ones")}
    assert seen["lengths"] == both(29), ("length symbols without a case", sorted(both(29) - seen["lengths"]))
    assert seen["distances"] == both(30), ("distance symbols without a case", sorted(both(30) - seen["distances"]))
    assert seen["through"] == {284, 285}, "258 comes through both symbols"
    assert seen["widest"] == 48, "no length and distance symbol of 15 + 5 + 15 + 13 bits: the longest a refill must hold"
    assert seen["cl_bits"] >= set(range(1, 8)), "a code-length-code length is never stated"
    assert frozenset(range(1, 8)) in seen["cl_sets"], "no code-length code holds all seven lengths at once"
    assert seen["pairs"] == {(a, b) for a in "sfd" for b in "sfd"}, "an ordered pair of block kinds is missing"
    lens = {n for _, n in seen["stored"]}
    assert 0 in lens and max(lens) == gx.MAX_STORED, "the empty and the largest stored block"
    assert seen["stored"] >= set(gx.stage_edges()), "a stored block at an edge of the staging window is missing"
    lane = {(length, distance) for length in gx.LANE_LENGTHS for distance in gx.LANE_DISTANCES}
    assert seen["repeats"] >= lane, ("lane-copy shapes without a case", sorted(lane - seen["repeats"]))
    # the stored LEN words that make the kernel hand bytes back below a window it has just staged: the refill before the block
    # header reaches at least 7 bytes past the header's byte (LEN - 1), LEN + 4 is where the reader goes on
    edge = gx.stage_bytes()
    assert {at for at, n in seen["stored"] if n < 3 and at + 4 < edge <= at + 6} and {at for at, n in seen["stored"] if n < 3 and at + 4 < 2 * edge <= at + 6}


def test_every_stream_reason_has_a_corrupt_case():
    """Each of the 12 reasons of ROCCO_BGZF_ERR_STREAM is zlib's verdict on the bad block of at least one corrupt file."""
    from rocco_amd import bam

    said = set()
    for label, raw, index, code in gx.corrupt_files():
        if code == gx.ERR_STREAM:
            _, lo, hi, _, _ = gx.blocks_of(raw)[index]
            said.add(gx.stream_reason(raw[lo:hi]))
    assert said == set(bam._STREAM_REASON_TEXT.values()) and len(said) == bam.BGZF_STREAM_REASONS
    for label in ("a length's extra bits", "a distance code", "a distance's extra bits", "a repeat code's extra bits", "the HLIT / HDIST / HCLEN word",
                  "the code-length code's lengths", "a stored LEN / NLEN"):
        assert any(have == f"the span ends inside {label}" for have, *_ in gx.corrupt_files()), label
    assert sum("48-bit symbol" in label for label, *_ in gx.corrupt_files()) == 3


def test_host_entry_on_the_valid_files():
    for label, raw in gx.valid_files():
        assert run_host(raw, label) == -1, label


def test_host_entry_on_the_corrupt_files():
    for label, raw, index, code in gx.corrupt_files():
        assert run_host(raw, label) == index, label


def test_host_entry_on_the_mutation_set():
    """2 000 seeded one-byte and one-bit mutations in one call: the same verdict as zlib on every block, none excluded."""
    raw = gx.mutation_file()
    want = gx.outcomes(raw)
    assert len(want) == gx.MUTATIONS
    run_host(raw, "mutations")
    codes = [code for code, _ in want]
    assert min(codes.count(c) for c in (0, gx.ERR_STREAM, gx.ERR_LENGTH, gx.ERR_CRC)) >= 10  # (every verdict is exercised)


def test_host_entry_on_the_long_mutation_set():
    """The second mutation set, of the census streams alone (long codes, every length and distance symbol, lane-copy shapes,
    block-kind pairs, stored blocks on window edges): the same verdict and the same reason as zlib on every block."""
    raw = gx.mutation_file_long()
    want = gx.outcomes(raw)
    assert len(want) == gx.MUTATIONS_LONG
    run_host(raw, "long mutations")
    codes = [code for code, _ in want]
    assert min(codes.count(c) for c in (0, gx.ERR_STREAM, gx.ERR_LENGTH, gx.ERR_CRC)) >= 10  # (every verdict is exercised)


def test_host_entry_on_the_turn_period_in_a_workgroups_order():
    """The period of the GPU launch-turn test, its blocks in the order one workgroup takes them (p, then p + cap mod 15, ...,
    twice round), through the host entry, whose one set of tables passes from block to block as a workgroup's does in LDS."""
    from rocco_amd import bam

    raw, half_way = gx.turn_period()
    rows = gx.blocks_of(raw)
    period = len(rows)
    ends = [at for at, *_ in rows[1:]] + [len(raw)]
    order = [k * (bam.BGZF_MAX_GRID % period) % period for k in range(2 * period)]
    assert sorted(order[:period]) == list(range(period)) and set(half_way) < set(order)
    turns = b"".join(raw[rows[p][0]: ends[p]] for p in order)
    refused = [k for k, (code, _) in enumerate(gx.outcomes(turns)) if code != 0]
    assert len(refused) == 2 * 6 and run_host(turns, "a workgroup's turns") == refused[0]


def test_rows_outside_the_buffers_are_refused():
    from rocco_amd import bam

    raw = gx.valid_files()[5][1]
    table = gx.table_of(raw)
    n_out = int(table[:, 2].sum())
    for column, value in ((0, -1), (1, len(raw) + 1), (2, 65537), (2, -1), (4, -1), (4, n_out), (0, int(table[0, 1]) + 1)):
        bad = table.copy()
        bad[0, column] = value
        out = np.full(n_out, gx.GUARD_BYTE, dtype=np.uint8)
        status, report = bam.inflate_blocks_host(raw, bad, out)
        assert status[0] == gx.ERR_TABLE and report["block"] == 0 and np.all(out[: int(table[0, 2])] == gx.GUARD_BYTE), (column, value)
    status, report = bam.inflate_blocks_host(b"", np.zeros((0, 5), dtype=np.int64), np.zeros(0, dtype=np.uint8))
    assert status.size == 0 and report["block"] == -1


def test_constants_agree_with_the_c_header():
    from rocco_amd import bam

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rocco_hip.h")).read()
    defined = {name: int(value) for name, value in re.findall(r"#define (ROCCO_BGZF_[A-Z_]+) (\d+)", text)}
    assert defined == {"ROCCO_BGZF_THREADS": bam.BGZF_THREADS, "ROCCO_BGZF_TABLE_COLUMNS": bam.BGZF_TABLE_COLUMNS,
                       "ROCCO_BGZF_MAX_ISIZE": bam.BGZF_MAX_ISIZE, "ROCCO_BGZF_REPORT": 4, "ROCCO_BGZF_STREAM_REASONS": bam.BGZF_STREAM_REASONS,
                       "ROCCO_BGZF_ERR_STREAM": bam.BGZF_ERR_STREAM, "ROCCO_BGZF_ERR_LENGTH": bam.BGZF_ERR_LENGTH,
                       "ROCCO_BGZF_ERR_CRC": bam.BGZF_ERR_CRC, "ROCCO_BGZF_ERR_TABLE": bam.BGZF_ERR_TABLE}
    (shift,) = re.findall(r"#define ROCCO_BGZF_MAX_GRID \(1 << (\d+)\)", text)  # (the grid cap, written as the kernel file wrote it)
    assert bam.BGZF_MAX_GRID == 1 << int(shift) == 1 << 20
    # (the cap is stated by the BGZF framing of inflate_core.h and used by the one launcher of the kernel file: neither writes the number)
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rocco_amd", "csrc")
    framing, source = open(os.path.join(csrc, "inflate_core.h")).read(), open(os.path.join(csrc, "bgzf_inflate.hip")).read()
    assert "kMaxGrid = ROCCO_BGZF_MAX_GRID;" in framing and "F::kMaxGrid" in source and "1 << 20" not in source + framing
    assert (bam.BGZF_ERR_STREAM, bam.BGZF_ERR_LENGTH, bam.BGZF_ERR_CRC, bam.BGZF_ERR_TABLE) == (gx.ERR_STREAM, gx.ERR_LENGTH, gx.ERR_CRC, gx.ERR_TABLE)
    assert bam.bgzf_shape() == {"threads": 64, "table_columns": 5, "max_isize": 65536, "stream_reasons": 12}
    assert sorted(bam._STREAM_REASON_TEXT) == list(range(1, bam.BGZF_STREAM_REASONS + 1))
    assert bam.DEFAULT_INFLATE == "host"


def test_block_table_and_mode_keyword(tmp_path):
    import rocco_amd
    from rocco_amd import bam

    raw = gx.valid_files()[-1][1]
    assert np.array_equal(bam.bgzf_block_table(gx.blocks_of(raw)), gx.table_of(raw))
    assert bam.bgzf_block_table([]).shape == (0, 5)
    assert rocco_amd.inflate_bgzf_device is bam.inflate_bgzf_device
    with pytest.raises(ValueError, match="inflate must be"):
        bam.read_alignment_file(str(tmp_path / "x.bam"), inflate="nonsense")
