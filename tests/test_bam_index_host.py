"""CPU: the host half of the indexed BAM read: the ``.bai`` parser of rocco_amd/bam_index.py
against the indexes htslib wrote (tests/golden/bam_index.npz, by tests/golden/make_golden_bam_index.py), the ranged BGZF front
of rocco_amd/bam.py, every refusal of both word for word, and the Python index writer of tests/bam_index_files.py pinned to
htslib."""
import os
import re
import struct

import numpy as np
import pytest

import bam_expected as bx
import bam_index_files as bif

FILES = ["mixed", "blocks", "longread", "header_only", "one_record", "unplaced_only", "cg", "decoy", "wide", "shared", "edges"]
CONTIGS = [("c0", 100000), ("c1", 100000), ("c2", 100000)]


def parsed(key):
    from rocco_amd import bam_index

    return bam_index.parse_bam_index(bif.golden_bai(key), key + ".bam.bai")


@pytest.mark.parametrize("key", FILES)
def test_spans_are_the_true_virtual_offsets_and_statistics_are_htslibs(key):
    """Per contig: the span equals the virtual offsets of its first record and of the end of its last, from the file's own
    record walk (bam_expected.walk); the statistics and the records-without-a-contig count equal htslib's dump."""
    from rocco_amd import bam_index

    _, meta = bif.golden()
    entry, index, facts = meta["files"][key], parsed(key), bif.facts(bif.golden_bam(key))
    assert index.n_ref == len(entry["refs"]) == facts["n_ref"]
    tid = facts["fields"]["tid"]
    for t, ref in enumerate(entry["refs"]):
        mine = np.flatnonzero(tid == t)
        assert np.array_equal(bif.golden()[0][f"itr_{key}_{t}"], mine)  # (htslib's iterator yields the contig's records, no others)
        span, stats = bam_index.contig_span(index, t), bam_index.contig_stats(index, t)
        if mine.size == 0:
            assert span is None and stats is None and not ref["has_stat"]
            continue
        v = facts["voffsets"]
        assert span == (int(v[mine[0]]), int(v[mine[-1] + 1])) == facts["spans"][t]
        assert ref["has_stat"] and stats == (ref["mapped"], ref["unmapped"]) == facts["stats"][t]
        assert span == bam_index.bins_span(index, t)  # the pseudo-bin's span is the min / max over the bins
    assert index.n_no_coor == entry["n_no_coor"] == int(np.count_nonzero(tid < 0))
    assert bam_index.contig_span(index, index.n_ref) is None and bam_index.contig_stats(index, -1) is None


def test_the_census_of_the_fixture_contigs():
    """Recomputed from the parsed indexes: contigs that begin inside a block, end inside one, share one, have no bins."""
    from rocco_amd import bam_index

    _, meta = bif.golden()
    census = {"begins_inside": [], "ends_inside": [], "share_a_block": [], "no_bins": []}
    for key in FILES:
        index = parsed(key)
        spans = [bam_index.contig_span(index, t) for t in range(index.n_ref)]
        for t, span in enumerate(spans):
            name = f"{key}:{meta['files'][key]['contigs'][t][0]}"
            if span is None:
                assert not index.bins[t]
                census["no_bins"].append(name)
                continue
            if span[0] & 0xFFFF:
                census["begins_inside"].append(name)
            if span[1] & 0xFFFF:
                census["ends_inside"].append(name)
            later = [u for u in range(t + 1, len(spans)) if spans[u] is not None]
            if later and span[1] & 0xFFFF and span[1] >> 16 == spans[later[0]][0] >> 16:
                census["share_a_block"].append(name)
    assert census == meta["census"] and all(len(v) >= 1 for v in census.values())
    assert "shared:chrA" in census["share_a_block"] and "shared:chrD" in census["share_a_block"]  # chrD lies inside one block
    assert "edges:chrB" not in census["ends_inside"] and "edges:chrA" not in census["begins_inside"]  # a seam on a block's end
    for key in meta["new_files"]:
        assert meta["files"][key]["bgzf_blocks"] >= 4 and len(meta["files"][key]["contigs"]) >= 4 and meta["files"][key]["n_no_coor"] > 0


@pytest.mark.parametrize("key", FILES)
def test_python_writer_is_pinned_to_htslib(key):
    """tests/bam_index_files.py: the spans, statistics and tail count it computes equal those of htslib's index; its own
    bins give the same min / max; it survives its own round trip."""
    from rocco_amd import bam_index

    theirs = parsed(key)
    mine = bam_index.parse_bam_index(bif.index_bytes(bif.golden_bam(key)), "mine.bai")
    assert mine.n_ref == theirs.n_ref and mine.n_no_coor == theirs.n_no_coor
    for t in range(theirs.n_ref):
        assert bam_index.contig_span(mine, t) == bam_index.contig_span(theirs, t)
        assert bam_index.contig_stats(mine, t) == bam_index.contig_stats(theirs, t)
        assert bam_index.bins_span(mine, t) == bam_index.bins_span(theirs, t)
    without = bam_index.parse_bam_index(bif.index_bytes(bif.golden_bam(key), pseudo=False, no_coor=False), "mine.bai")
    assert without.n_no_coor is None
    for t in range(theirs.n_ref):
        assert bam_index.contig_span(without, t) == bam_index.contig_span(theirs, t) and bam_index.contig_stats(without, t) is None
    assert bif.reg2bin(0, 1) == 4681 and bif.reg2bin(16383, 16385) == 585 and bif.reg2bin(0, 1 << 29) == 0


def small_index():
    return bif.index_bytes(bif.synthetic_bam(CONTIGS, [(0, 60), (0, 70), (2, 64)], cuts=(60,), tail=1))


def test_parser_refusals_word_for_word():
    from rocco_amd import bam_index

    good = small_index()
    index = bam_index.parse_bam_index(good, "x.bai")
    assert index.n_ref == 3 and index.n_no_coor == 1 and index.pseudo[1] is None and index.bins[1] == {}
    size = len(good)

    def refused(raw, words):
        with pytest.raises(ValueError) as info:
            bam_index.parse_bam_index(raw, "x.bai")
        assert str(info.value) == words

    refused(b"BAI", "x.bai: the header at file offset 0: 8 bytes from there leave the file (3 bytes)")
    refused(b"BAM\x01" + good[4:], "x.bai: the header at file offset 0: magic b'BAM\\x01' where b'BAI\\x01' belongs (not a .bai index)")
    refused(good[:4] + struct.pack("<i", -2) + good[8:], "x.bai: the header at file offset 4: n_ref is negative (-2)")
    refused(good[:4] + struct.pack("<i", 4) + good[8:-8], f"x.bai: n_bin of reference 3 at file offset {size - 8}: 4 bytes from there leave the file ({size - 8} bytes)")
    refused(good[:8] + struct.pack("<i", 1 << 20) + good[12:],
            f"x.bai: the bins of reference 0 at file offset 12: {8 << 20} bytes from there leave the file ({size} bytes)")
    refused(good[:8] + struct.pack("<i", -1) + good[12:], "x.bai: n_bin of reference 0 at file offset 8: it is negative (-1)")
    (bin0,) = struct.unpack_from("<I", good, 12)
    refused(good[:16] + struct.pack("<i", 1 << 24) + good[20:],
            f"x.bai: the chunks of bin {bin0} of reference 0 at file offset 20: {16 << 24} bytes from there leave the file ({size} bytes)")
    refused(good[:16] + struct.pack("<i", -3) + good[20:], f"x.bai: bin {bin0} of reference 0 at file offset 12: n_chunk is negative (-3)")
    begin, end = struct.unpack_from("<QQ", good, 20)
    refused(good[:20] + struct.pack("<QQ", end + 5, end) + good[36:],
            f"x.bai: chunk 0 of bin {bin0} of reference 0 at file offset 20: it ends at virtual offset {end}, before its begin {end + 5}")
    # the pseudo-bin of reference 0: found by its number
    at = good.index(struct.pack("<Ii", bam_index.PSEUDO_BIN, 2))
    refused(good[:at + 4] + struct.pack("<i", 1) + good[at + 8: at + 24] + good[at + 40:],
            f"x.bai: the pseudo-bin 37450 of reference 0 at file offset {at}: it has 1 chunks where 2 belong")
    v_begin, v_end = struct.unpack_from("<QQ", good, at + 8)
    refused(good[:at + 8] + struct.pack("<QQ", v_end + 1, v_end) + good[at + 24:],
            f"x.bai: the pseudo-bin 37450 of reference 0 at file offset {at + 8}: its span ends at virtual offset {v_end}, before its begin {v_end + 1}")
    # the linear index: its length is checked
    n_intv_at = at + 40
    (n_intv,) = struct.unpack_from("<i", good, n_intv_at)
    assert n_intv == index.n_intv[0] >= 1
    refused(good[:n_intv_at] + struct.pack("<i", 1 << 26) + good[n_intv_at + 4:],
            f"x.bai: the linear index of reference 0 at file offset {n_intv_at + 4}: {8 << 26} bytes from there leave the file ({size} bytes)")
    refused(good[:n_intv_at] + struct.pack("<i", -1) + good[n_intv_at + 4:], f"x.bai: n_intv of reference 0 at file offset {n_intv_at}: it is negative (-1)")
    refused(good[:n_intv_at + 2], f"x.bai: n_intv of reference 0 at file offset {n_intv_at}: 4 bytes from there leave the file ({n_intv_at + 2} bytes)")
    # a file that ends before n_no_coor is whole
    assert bam_index.parse_bam_index(good[:-8], "x.bai").n_no_coor is None and bam_index.parse_bam_index(good[:-3], "x.bai").n_no_coor is None


def test_finding_the_index_as_htslib_does(tmp_path):
    from rocco_amd import bam_index

    raw = bif.synthetic_bam(CONTIGS, [(0, 60), (1, 70)])
    bam_path = str(tmp_path / "a.bam")
    with open(bam_path, "wb") as handle:
        handle.write(raw)
    assert bam_index.open_bam_index(bam_path) is None
    with open(str(tmp_path / "a.bam.csi"), "wb") as handle:  # a .csi index alone: not read, the file takes the whole-file route
        handle.write(b"CSI\x01" + bytes(24))
    assert bam_index.open_bam_index(bam_path) is None and bam_index.bam_index_path(bam_path) is None
    with open(str(tmp_path / "a.bai"), "wb") as handle:
        handle.write(bif.index_bytes(raw))
    second = bam_index.open_bam_index(bam_path)
    assert second.name == str(tmp_path / "a.bai") and bam_index.open_bam_index(bam_path) is second  # (cached)
    with open(bam_path + ".bai", "wb") as handle:
        handle.write(bif.index_bytes(raw, pseudo=False))
    first = bam_index.open_bam_index(bam_path)
    assert first.name == bam_path + ".bai" and first.pseudo == [None] * 3  # <path>.bai comes before the replaced extension
    os.utime(bam_path + ".bai", ns=(5, 5))
    assert bam_index.open_bam_index(bam_path) is not first  # keyed on (path, size, mtime)
    bam_index.clear_bam_index_cache()
    assert bam_index.open_bam_index(bam_path) is not second
    with open(bam_path + ".bai", "wb") as handle:
        handle.write(b"nonsense")
    with pytest.raises(ValueError, match=re.escape(f"{bam_path}.bai: the header at file offset 0: magic b'nons'")):
        bam_index.open_bam_index(bam_path)


@pytest.mark.parametrize("key", FILES)
def test_ranged_front_gives_the_contigs_bytes(key):
    """The blocks between a span's virtual offsets, minus the skip and cut at the keep, inflate to exactly the contig's records."""
    from rocco_amd import bam, bam_index

    raw = bif.golden_bam(key)
    facts, index = bif.facts(raw), parsed(key)
    data, _ = bx.inflate(raw)
    edges = np.concatenate([facts["offsets"], [len(data)]])
    tid = facts["fields"]["tid"]
    whole = bam._bgzf_blocks(memoryview(raw), key)
    for t in range(index.n_ref):
        span = bam_index.contig_span(index, t)
        if span is None:
            continue
        blocks, skip, keep = bam._bgzf_span_blocks(memoryview(raw), key, f"t{t}", *span)
        assert all(b in whole for b in blocks) and blocks == [b for b in whole if blocks[0][0] <= b[0] <= blocks[-1][0]]
        got = b"".join(bam._inflate_block(memoryview(raw), key, i, b) for i, b in enumerate(blocks))
        got = got[skip: len(got) - (blocks[-1][4] - keep)]
        mine = np.flatnonzero(tid == t)
        assert got == data[int(edges[mine[0]]): int(edges[mine[-1] + 1])]


def test_ranged_front_edges_and_refusals_word_for_word():
    from rocco_amd import bam

    raw = bif.synthetic_bam(CONTIGS, [(0, 60), (0, 70), (1, 64), (2, 80)], cuts=(60, 130, 194))
    table = bif.block_table(raw)
    assert len(table) == 5 and table[-1][2] == 0  # four data blocks and the end-of-file marker
    view, size = memoryview(raw), len(raw)
    at = [row[0] for row in table]
    rows = bam._bgzf_blocks(view, "f.bam")
    # skip == ISIZE: htslib may point at a block's end; the block contributes nothing
    blocks, skip, keep = bam._bgzf_span_blocks(view, "f.bam", "c1", at[1] << 16 | table[1][2], at[3] << 16)
    assert blocks == rows[1:3] and skip == table[1][2] and keep == table[2][2]
    # v_end & 0xFFFF == 0 leaves the last block out; a span to the file's end is legal; so is an empty span
    assert bam._bgzf_span_blocks(view, "f.bam", "c2", at[3] << 16, size << 16) == (rows[3:], 0, 0)
    assert bam._bgzf_span_blocks(view, "f.bam", "c2", at[3] << 16, at[4] << 16) == (rows[3:4], 0, table[3][2])
    assert bam._bgzf_span_blocks(view, "f.bam", "c0", at[2] << 16, at[2] << 16) == ([], 0, 0)
    assert bam._bgzf_span_blocks(view, "f.bam", "c0", at[2] << 16 | 7, at[2] << 16 | 7) == (rows[2:3], 7, 7)
    assert bam._bgzf_span_blocks(view, "f.bam", "c0", at[0] << 16 | 5, at[1] << 16 | 9) == (rows[0:2], 5, 9)

    def refused(v_begin, v_end, words):
        with pytest.raises(ValueError) as info:
            bam._bgzf_span_blocks(view, "f.bam", "c1", v_begin, v_end)
        assert str(info.value) == words

    def v(offset):
        return f"virtual offset {offset} ({offset >> 16} << 16 | {offset & 0xFFFF}) of the index"

    refused(at[2] << 16, at[1] << 16, f"f.bam: contig c1: {v(at[1] << 16)} ends the span before its begin, virtual offset {at[2] << 16}")
    refused((size + 3) << 16, (size + 3) << 16 | 1, f"f.bam: contig c1: {v((size + 3) << 16)} points outside the file ({size} bytes)")
    refused(at[1] << 16, (size + 40) << 16, f"f.bam: contig c1: {v((size + 40) << 16)} points outside the file ({size} bytes)")
    refused(at[1] << 16, size << 16 | 4, f"f.bam: contig c1: {v(size << 16 | 4)} points outside the file ({size} bytes)")
    refused(at[1] << 16 | (table[1][2] + 1), at[3] << 16, f"f.bam: contig c1: {v(at[1] << 16 | (table[1][2] + 1))} points past the block's ISIZE ({table[1][2]})")
    refused(at[1] << 16, at[2] << 16 | (table[2][2] + 2), f"f.bam: contig c1: {v(at[2] << 16 | (table[2][2] + 2))} points past the block's ISIZE ({table[2][2]})")
    refused(at[1] << 16, (at[2] + 1) << 16 | 3,
            f"f.bam: contig c1: {v((at[2] + 1) << 16 | 3)} names no block: the blocks from the span's begin pass it, the next begins at file offset {at[3]}")
    refused(at[1] << 16, (at[2] + 1) << 16,
            f"f.bam: contig c1: {v((at[2] + 1) << 16)} names no block: the blocks from the span's begin pass it, the next begins at file offset {at[3]}")
    # a begin that names no block header: the words of `_bgzf_blocks`, the blocks counted from the span
    with pytest.raises(ValueError) as info:
        bam._bgzf_span_blocks(view, "f.bam", "c1", (at[1] + 1) << 16, at[3] << 16)
    assert str(info.value) == f"f.bam: BGZF block 0 at file offset {at[1] + 1} (blocks counted from the span of contig c1): bad header (no gzip magic)"
    with pytest.raises(ValueError, match=re.escape(f"f.bam: BGZF block 4 at file offset {at[4]}: the file ends inside the block (20 of 28 bytes)")):
        bam._bgzf_blocks(view[:size - 8], "f.bam")  # (the shared block parser keeps the whole-file front's words)
    with pytest.raises(ValueError) as info:
        bam._bgzf_span_blocks(view[:size - 8], "f.bam", "c2", at[3] << 16, at[4] << 16 | 1)
    assert str(info.value) == (f"f.bam: BGZF block 1 at file offset {at[4]} (blocks counted from the span of contig c2): "
                               "the file ends inside the block (20 of 28 bytes)")


def test_leading_blocks_read_the_header_without_walking_the_file():
    from rocco_amd import bam

    raw = bx.bam_bytes("blocks")
    lazy = bam._LeadingBlocks(memoryview(raw), "b.bam")
    contigs, entry0 = bam._header_from_leading_blocks(memoryview(raw), "b.bam", lazy)
    whole = bam._bgzf_blocks(memoryview(raw), "b.bam")
    assert (contigs, entry0) == bam._header_from_leading_blocks(memoryview(raw), "b.bam", whole)
    assert 1 <= len(lazy.rows) <= 2 < len(whole) and lazy.rows == whole[: len(lazy.rows)]
    # a header in many small blocks, and a file that ends inside it
    data, _ = bx.inflate(raw)
    small = bx.bgzf_compress(data[: entry0 + 100], cuts=range(7, entry0 + 100, 7))
    assert bam._header_from_leading_blocks(memoryview(small), "s.bam", bam._LeadingBlocks(memoryview(small), "s.bam")) == (contigs, entry0)
    cut = bx.bgzf_compress(data[: entry0 - 3], cuts=(10,))
    with pytest.raises(ValueError, match=r"c\.bam: BAM header: the stream ends inside"):
        bam._header_from_leading_blocks(memoryview(cut), "c.bam", bam._LeadingBlocks(memoryview(cut), "c.bam"))


def test_span_groups_rule():
    """Groups stay under the budget, share one header length, keep the reference ids from descending; a stream that alone
    exceeds the budget is a group of its own."""
    from rocco_amd import bam

    def stream(size, tid=0, n_ref=3):
        s = bam._Stream()
        s.size, s.tid, s.n_ref = size, tid, n_ref
        return s

    groups = lambda streams, budget: list(bam._span_groups(streams, budget))  # noqa: E731
    assert groups([stream(10) for _ in range(5)], 100) == [(0, 5)]
    assert groups([stream(40) for _ in range(5)], 100) == [(0, 2), (2, 4), (4, 5)]
    assert groups([stream(10), stream(500), stream(10), stream(10)], 100) == [(0, 1), (1, 2), (2, 4)]
    assert groups([stream(500), stream(10)], 100) == [(0, 1), (1, 2)]
    assert groups([stream(10, 0), stream(10, 1), stream(0, 0), stream(10, 2), stream(10, 1)], 100) == [(0, 4), (4, 5)]
    assert groups([stream(10, 0), stream(10, 0, n_ref=4)], 100) == [(0, 1), (1, 2)]
    assert groups([stream(0, 2), stream(10, 0)], 100) == [(0, 2)] and groups([], 100) == []


def test_constants_exports_and_the_header():
    import rocco_amd
    from rocco_amd import bam, bam_index

    text = open(os.path.join(os.path.dirname(bx.HERE), "include", "rocco_hip.h")).read()
    defined = dict(re.findall(r"#define (ROCCO_BAM_[A-Z_]+) (\d+)", text))
    assert int(defined["ROCCO_BAM_ERR_SEAM"]) == bam.ERR_SEAM == 12 and int(defined["ROCCO_BAM_ERR_SPAN_TID"]) == bam.ERR_SPAN_TID == 13
    assert "rocco_hip_bam_stream_firsts" in text and bam.USE_INDEX is True and bam.DEFAULT_BATCH_BYTES == 2 << 30
    for name in ("read_alignment_spans", "IndexedAlignmentFile"):
        assert getattr(rocco_amd, name) is getattr(bam, name)
    for name in ("open_bam_index", "contig_span", "contig_stats"):
        assert getattr(rocco_amd, name) is getattr(bam_index, name)
    assert issubclass(bam.IndexedAlignmentFile, rocco_amd.readtracks.AlignmentFileRecords)
