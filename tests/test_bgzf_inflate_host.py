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

    for label, cdata, data in gx.hand_streams():
        assert zlib.decompress(cdata, wbits=-15) == data, label
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
