"""CPU: the host half of the BAM reader (rocco_amd/bam.py: BGZF inflate, the BAM header) and the NumPy statement the GPU
tests hold the kernels against (tests/bam_expected.py), which must itself equal htslib's own decoding of every fixture
(tests/golden/bam_files.npz, written by tests/golden/make_golden_bam_files.py)."""
import numpy as np
import pytest

import bam_expected as bx

FILES = ["mixed", "blocks", "longread", "header_only", "one_record", "unplaced_only", "cg", "decoy"]


@pytest.mark.parametrize("key", FILES)
def test_statement_equals_htslibs_dump(key):
    """Inflate, header, sequential walk and fields of the NumPy statement against what htslib decoded, record by record.  The
    record of `cg` whose CIGAR lives in a CG tag is flagged, and only its `end` and `qlen` (which need that CIGAR) differ."""
    _, meta = bx.golden()
    data, _ = bx.inflate(bx.bam_bytes(key))
    _, contigs, entry0 = bx.header(data)
    assert [list(c) for c in contigs] == meta["sizes"][:3] and entry0 == meta["files"][key]["first_record"]
    offsets, end, why, _ = bx.walk(data, entry0)
    want = bx.dump(key)
    assert why == 0 and end == len(data) and offsets.size == want["tid"].size == meta["files"][key]["records"]
    got, (code, record) = bx.fields(data, offsets, len(contigs))
    if key == "cg":
        assert code == bx.ERR_CG_TAG and want["qlen"][record] == 33000 and want["end"][record] - want["pos"][record] == 66000
        keep = np.arange(offsets.size) != record
    else:
        assert code == 0 and record == -1
        keep = np.ones(offsets.size, dtype=bool)
    for name, dtype in bx.FIELDS:
        assert got[name].dtype == want[name].dtype == dtype
        mask = keep if name in ("end", "qlen") else slice(None)
        assert np.array_equal(got[name][mask], want[name][mask]), (key, name)
    assert np.all(np.diff(np.where(want["tid"] < 0, len(contigs), want["tid"])) >= 0)


def test_fixtures_cover_what_the_walk_must_survive():
    _, meta = bx.golden()
    files = meta["files"]
    assert files["blocks"]["bgzf_blocks"] >= 4 and files["header_only"]["records"] == 0 and files["one_record"]["records"] == 1
    data, starts = bx.inflate(bx.bam_bytes("blocks"))
    offsets, _, _, _ = bx.walk(data, bx.header(data)[2])
    inside_word = [s for s in starts if 0 < s - offsets[np.searchsorted(offsets, s) - 1] < 4]
    assert inside_word, "a BGZF block boundary must fall inside a block_size word"
    assert np.all(bx.dump("unplaced_only")["tid"] == -1) and (bx.dump("mixed")["tid"] == -1).sum() == 40
    assert bx.dump("longread")["qlen"].max() == 3000
    for key in FILES:
        assert files[key]["wrong_guesses_default"] == 0 or key == "decoy"


def test_predicate_accepts_the_decoy():
    """The fake records in the B:C tag pass the predicate; at the stated segment size the first of them is its segment's
    guess although no record starts there; at the default size every other fixture guesses every segment right."""
    _, meta = bx.golden()
    data, _ = bx.inflate(bx.bam_bytes("decoy"))
    _, contigs, entry0 = bx.header(data)
    at, S = meta["decoy_offset"], meta["decoy_segment_bytes"]
    offsets, _, _, _ = bx.walk(data, entry0)
    assert at not in set(offsets.tolist()) and bx.plausible_chain(data, at, len(contigs))
    assert bx.guesses(data, entry0, len(contigs), S)[at // S] == at and bx.true_entries(data, entry0, S)[at // S] != at
    assert bx.wrong_guesses(data, entry0, len(contigs), S) >= 1
    for o in offsets[:50]:
        assert bx.plausible_chain(data, int(o), len(contigs))
    assert not bx.plausible_chain(data, int(offsets[3]) + 1, len(contigs))
    small, _ = bx.inflate(bx.bam_bytes("one_record"))
    assert bx.wrong_guesses(small, bx.header(small)[2], 3, bx.DEFAULT_SEGMENT_BYTES) == 0


def test_inflate_bgzf_matches_and_checks(tmp_path):
    from rocco_amd import bam

    for key in ("blocks", "mixed", "header_only"):
        raw = bx.bam_bytes(key)
        want, _ = bx.inflate(raw)
        got = bam.inflate_bgzf(raw)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.tobytes() == want
        assert bam.inflate_bgzf(bx.write_bam(tmp_path, key), threads=3).tobytes() == want
        for slab_bytes in (1, 1000, 4096, 70000, 1 << 30):
            slabs = list(bam.inflate_bgzf(raw, slab_bytes=slab_bytes))
            assert b"".join(s.tobytes() for s in slabs) == want
            assert all(s.size >= slab_bytes for s in slabs[:-1]) and all(s.size < slab_bytes + 0xFF00 for s in slabs)
    raw = bx.bam_bytes("blocks")
    want, starts = bx.inflate(raw)
    assert len(starts) >= 4
    assert len(list(bam.inflate_bgzf(raw, slab_bytes=1))) == len(starts) - 1  # (one block per slab, the end-of-file marker with the last)
    # an extra subfield in front of BC; no end-of-file marker
    again = bx.bgzf_compress(want, cuts=[1000, 5000, 70001], eof=False, extra_first=b"XY" + (5).to_bytes(2, "little") + b"hello")
    assert bam.inflate_bgzf(again).tobytes() == want
    assert bam.inflate_bgzf(b"").size == 0


def test_inflate_bgzf_errors_name_block_and_offset():
    from rocco_amd import bam

    want, _ = bx.inflate(bx.bam_bytes("blocks"))
    first = bx.bgzf_block(want[:3000])
    raw = first + bx.bgzf_block(want[3000:9000]) + bx.EOF_BLOCK
    flipped = bytearray(raw)
    flipped[len(first) + len(bx.bgzf_block(want[3000:9000])) - 8] ^= 1  # a bit of the second block's CRC32
    with pytest.raises(ValueError, match=rf"BGZF block 1 at file offset {len(first)}: CRC32 mismatch"):
        bam.inflate_bgzf(bytes(flipped))
    longer = bytearray(raw)
    longer[len(first) + len(bx.bgzf_block(want[3000:9000])) - 4] ^= 1  # ISIZE
    with pytest.raises(ValueError, match=rf"BGZF block 1 at file offset {len(first)}: length mismatch"):
        bam.inflate_bgzf(bytes(longer))
    with pytest.raises(ValueError, match=rf"BGZF block 1 at file offset {len(first)}: the file ends inside the block"):
        bam.inflate_bgzf(raw[: len(first) + 100])
    with pytest.raises(ValueError, match=rf"BGZF block 1 at file offset {len(first)}: the file ends inside the block header"):
        bam.inflate_bgzf(raw[: len(first) + 5])
    with pytest.raises(ValueError, match=r"BGZF block 0 at file offset 0: bad header \(no gzip magic\)"):
        bam.inflate_bgzf(b"\x1f\x8c" + raw[2:])
    with pytest.raises(ValueError, match=r"BGZF block 0 at file offset 0: bad header \(FLG.FEXTRA"):
        bam.inflate_bgzf(raw[:3] + b"\0" + raw[4:])
    with pytest.raises(ValueError, match=r"BGZF block 0 at file offset 0: bad header \(no BC subfield\)"):
        bam.inflate_bgzf(raw[:12] + b"XC" + raw[14:])
    garbage = bytearray(raw)
    garbage[20] ^= 0xFF  # inside the deflate data of block 0
    with pytest.raises(ValueError, match=r"BGZF block 0 at file offset 0"):
        bam.inflate_bgzf(bytes(garbage))


def test_parse_bam_header_and_its_errors():
    from rocco_amd import bam

    for key in ("mixed", "header_only"):
        data, _ = bx.inflate(bx.bam_bytes(key))
        assert bam.parse_bam_header(data) == bx.header(data)
        assert bam.parse_bam_header(np.frombuffer(data, dtype=np.uint8)) == bx.header(data)
    made = bx.make_header([("a", 10), ("chrLong", 2 ** 31 - 1)], "@HD\tVN:1.6\n")
    assert bam.parse_bam_header(made) == ("@HD\tVN:1.6\n", [("a", 10), ("chrLong", 2 ** 31 - 1)], len(made))
    assert bam.parse_bam_header(bx.make_header([])) == ("", [], 12)
    with pytest.raises(ValueError, match="magic"):
        bam.parse_bam_header(b"BAM\x02" + made[4:])
    for cut in (2, 6, 12, len(made) - 30, len(made) - 1):
        with pytest.raises(ValueError, match="ends inside"):
            bam.parse_bam_header(made[:cut])
    bad = bytearray(made)
    bad[4:8] = (-5).to_bytes(4, "little", signed=True)
    with pytest.raises(ValueError, match="l_text is negative"):
        bam.parse_bam_header(bytes(bad))
    bad = bytearray(bx.make_header([("a", 10)]))
    bad[12:16] = (0).to_bytes(4, "little")
    with pytest.raises(ValueError, match="l_name of contig 0"):
        bam.parse_bam_header(bytes(bad))
    bad = bytearray(bx.make_header([("a", 10)]))
    bad[17] = 65
    with pytest.raises(ValueError, match="NUL-terminated"):
        bam.parse_bam_header(bytes(bad))


def test_exports_and_the_stub_stay():
    import rocco_amd
    from rocco_amd import bam, readtracks

    for name in ("inflate_bgzf", "parse_bam_header", "read_alignment_file", "get_bam_chrom_reads", "clear_alignment_cache"):
        assert getattr(rocco_amd, name) is getattr(bam, name)
    assert callable(bam._get_bam_count_metadata) and bam.GUESS_DEPTH == bx.GUESS_DEPTH and bam.DEFAULT_SEGMENT_BYTES == bx.DEFAULT_SEGMENT_BYTES
    assert [getattr(bam, n) for n in ("ERR_BLOCK_SIZE", "ERR_TRUNCATED", "ERR_SIZES", "ERR_READ_NAME", "ERR_REF_ID", "ERR_CIGAR_SEQ",
                                      "ERR_POSITION", "ERR_END", "ERR_CG_TAG", "ERR_ORDER", "ERR_OFFSET")] == list(range(1, 12))
    with pytest.raises(RuntimeError, match="rocco_amd does not decode BAM files"):
        readtracks.get_bam_chrom_reads("x.bam")
    with pytest.raises(FileNotFoundError, match="BAM file not found: /nowhere/x.bam"):
        bam.get_bam_chrom_reads("/nowhere/x.bam", "chr1", "/nowhere/t.sizes", 50)


def test_header_constants_agree_with_the_c_header():
    import os
    import re

    text = open(os.path.join(os.path.dirname(bx.HERE), "include", "rocco_hip.h")).read()
    defined = dict(re.findall(r"#define (ROCCO_BAM_[A-Z_]+) (\d+)", text))
    assert int(defined["ROCCO_BAM_RUNOFF_BYTES"]) == bx.RUNOFF_BYTES
    assert int(defined["ROCCO_BAM_GUESS_DEPTH"]) == bx.GUESS_DEPTH and int(defined["ROCCO_BAM_SEGMENT_BYTES"]) == bx.DEFAULT_SEGMENT_BYTES
    for name in ("BLOCK_SIZE", "TRUNCATED", "SIZES", "READ_NAME", "REF_ID", "CIGAR_SEQ", "POSITION", "END", "CG_TAG", "ORDER", "OFFSET"):
        assert int(defined[f"ROCCO_BAM_ERR_{name}"]) == getattr(bx, f"ERR_{name}")


def test_one_slab_rule():
    """`_slab_groups`, the one statement of where slabs are cut: every block once and in order, every group but the last at least
    ``slab_bytes`` inflated bytes, and `inflate_bgzf` yields one slab of each group's inflated size."""
    from rocco_amd import bam

    want, _ = bx.inflate(bx.bam_bytes("blocks"))
    empty = bx.bgzf_block(b"")
    middle = bx.bgzf_compress(want[:3000], cuts=(700, 1400), eof=False) + empty + empty + bx.bgzf_compress(want[3000:9000], cuts=(5000,))
    for raw in (bx.bam_bytes("blocks"), middle):
        blocks = bam._bgzf_blocks(memoryview(raw), "<bytes>")
        sizes = [b[4] for b in blocks]
        for slab_bytes in (None, 1, 1000, 70000):
            groups = list(bam._slab_groups(blocks, slab_bytes))
            assert [k for first, last in groups for k in range(first, last)] == list(range(len(blocks)))
            assert all(last > first for first, last in groups)
            inflated = [sum(sizes[first:last]) for first, last in groups]
            if slab_bytes is None:
                assert len(groups) == 1
                slabs = [bam.inflate_bgzf(raw)]
            else:
                assert all(n >= slab_bytes for n in inflated[:-1])
                slabs = list(bam.inflate_bgzf(raw, slab_bytes=slab_bytes))
            assert [int(s.size) for s in slabs] == inflated
    groups = list(bam._slab_groups(bam._bgzf_blocks(memoryview(middle), "<bytes>"), 1))
    assert (2, 5) in groups and groups[-1][1] - groups[-1][0] == 2  # (the empty blocks and the end-of-file marker go with the slab before)
