"""Host: the staging that the BAM and the bigWig reader share (rocco_amd/inflate.py: `SpanList`, `upload_blocks`) and the two
layouts built on it (`bam._group_layout`, `bigwig._chrom_layout`), against layouts built here from the block rows alone.  No
GPU: the "upload" goes to the CPU device, where the views of the uploaded tensor are read back as they are."""
import zlib

import numpy as np

import bgzf_expected as gx
import bigwig_files as bf


def bgzf_file(n_blocks):
    """(the bytes of a BGZF file of `n_blocks` blocks of 90 .. 700 bytes, their rows, the payloads)."""
    payloads = [gx.text_bytes(300 + 131 * k, 40 + k) for k in range(n_blocks)]
    raw = b"".join(gx.packed(data, level=(1, 6, 9)[k % 3]) for k, data in enumerate(payloads))
    return raw, gx.blocks_of(raw), payloads


def uploaded(table, spans):
    import torch

    from rocco_amd import inflate

    table_t, comp_t = inflate.upload_blocks(table, spans.spans, spans.n_comp, "cpu")
    assert table_t.dtype == torch.int64 and comp_t.dtype == torch.uint8
    return table_t.numpy().reshape(-1, 5), comp_t.numpy().tobytes()


def stream(raw, blocks, skip, keep):
    from rocco_amd import bam

    s = bam._Stream()
    s.path, s.contig, s.tid, s.n_ref, s.index_name, s.raw, s.blocks, s.skip, s.keep = "x.bam", "chrA", 0, 1, "x.bam.bai", raw, blocks, skip, keep
    s.size = sum(b[4] for b in blocks) - skip - (blocks[-1][4] - keep) if blocks else 0
    return s


def test_one_contiguous_slab():
    """What `_inflate_slabs_device` stages for a slab: one span from the first block's deflate data to the last one's end."""
    from rocco_amd import bam, inflate

    raw, blocks, payloads = bgzf_file(6)
    group = blocks[1:5]
    base, end = group[0][1], group[-1][2]
    spans = inflate.SpanList()
    assert spans.add(memoryview(raw), base, end) == 0 and spans.n_comp == end - base and len(spans.spans) == 1
    table, comp = uploaded(bam.bgzf_block_table(group, base), spans)
    assert comp == raw[base:end] and np.array_equal(table, bam.bgzf_block_table(group, base))
    for (lo, hi, isize, crc, offset), data in zip(table.tolist(), payloads[1:5]):  # (and the table means what rocco_hip.h says)
        assert zlib.decompress(comp[lo:hi], wbits=-15) == data and (isize, crc) == (len(data), zlib.crc32(data))
    assert table[:, 4].tolist() == np.concatenate([[0], np.cumsum([len(d) for d in payloads[1:4]])]).tolist()


def test_two_streams_share_their_boundary_block_and_neighbours_ride_in_one_span():
    from rocco_amd import bam

    raw, blocks, payloads = bgzf_file(9)
    view, other = memoryview(raw), memoryview(bytes(raw))  # (the same bytes as another file's: another object)
    a, b = stream(view, blocks[0:3], 5, 10), stream(view, blocks[2:5], 10, 33)  # (b begins in the block a ends in)
    far, nothing, elsewhere = stream(view, blocks[7:9], 0, 7), stream(view, [], 0, 0), stream(other, blocks[0:1], 1, 2)
    table, spans, owner, slices = bam._group_layout([a, b, far, nothing, elsewhere])
    rows = blocks[0:5] + blocks[7:9] + blocks[0:1]  # (one row for blocks[2])
    assert [(s, index, at) for s, index, at in owner] == [(a, 0, blocks[0][0]), (a, 1, blocks[1][0]), (a, 2, blocks[2][0]), (b, 1, blocks[3][0]),
                                                          (b, 2, blocks[4][0]), (far, 0, blocks[7][0]), (far, 1, blocks[8][0]),
                                                          (elsewhere, 0, blocks[0][0])]
    starts = np.concatenate([[0], np.cumsum([r[4] for r in rows])]).tolist()
    assert table[:, 2].tolist() == [r[4] for r in rows] and table[:, 3].tolist() == [r[3] for r in rows] and table[:, 4].tolist() == starts[:-1]
    assert slices == [(starts[0] + 5, starts[2] + 10), (starts[2] + 10, starts[4] + 33), (starts[5] + 0, starts[6] + 7), (0, 0),
                      (starts[7] + 1, starts[7] + 2)]
    # neighbouring blocks lie 26 bytes apart (8 of trailer, 18 of header) and ride in one span with what lies between; blocks
    # 5 and 6 lie between blocks 4 and 7 (more than 64 bytes): a new span; the other file's block: a new span, whatever its offset
    assert all(blocks[k + 1][1] - blocks[k][2] == 26 for k in range(8)) and blocks[7][1] - blocks[4][2] > 64
    want = [(view, blocks[0][1], blocks[4][2] - blocks[0][1]), (view, blocks[7][1], blocks[8][2] - blocks[7][1]),
            (other, blocks[0][1], blocks[0][2] - blocks[0][1])]
    assert len(spans.spans) == 3 and all(got[0] is src and tuple(got[1:]) == (lo, size) for got, (src, lo, size) in zip(spans.spans, want))
    assert spans.n_comp == sum(size for _, _, size in want)
    up_table, comp = uploaded(table, spans)
    assert np.array_equal(up_table, table) and comp == b"".join(bytes(src[lo: lo + size]) for src, lo, size in want)
    for (lo, hi, isize, crc, offset), row in zip(table.tolist(), rows):
        assert comp[lo:hi] == raw[row[1]: row[2]]


def test_the_gap_that_still_rides_along():
    from rocco_amd import inflate

    raw = memoryview(bytes(range(256)) * 4)
    spans = inflate.SpanList()
    assert spans.add(raw, 10, 20, 64) == 0
    assert spans.add(raw, 84, 90, 64) == 74 and len(spans.spans) == 1  # (64 bytes behind: rides, and the 64 with it)
    assert spans.add(raw, 155, 160, 64) == 80 and len(spans.spans) == 2  # (65 bytes behind: a span of its own)
    assert spans.add(raw, 160, 170, 0) == 85 and len(spans.spans) == 2  # (exactly adjacent)
    assert spans.add(raw, 171, 180, 0) == 95 and len(spans.spans) == 3  # (one byte behind, max_gap 0)
    assert spans.add(raw, 100, 110, 64) == 104 and len(spans.spans) == 4  # (in front of the span before: never merged)
    assert [s[1:] for s in spans.spans] == [[10, 80], [155, 15], [171, 9], [100, 10]] and spans.n_comp == 114
    _, comp = uploaded(np.zeros((0, 5), dtype=np.int64), spans)
    assert comp == bytes(raw[10:90]) + bytes(raw[155:170]) + bytes(raw[171:180]) + bytes(raw[100:110])


def test_three_bigwig_files_coalesce_within_a_file_and_only_when_adjacent(tmp_path):
    from rocco_amd import bigwig

    bigwig.clear_bigwig_cache()
    chroms = [("chr1", 10 ** 6), ("chr2", 10 ** 6)]
    ones, twos = bf.fixed_sections(0, 5, 30, seed=3), bf.fixed_sections(1, 2, 30, seed=4)
    records = [bf.write_bigwig(str(tmp_path / "a.bw"), chroms, ones[:3], level=6),
               bf.write_bigwig(str(tmp_path / "b.bw"), chroms, ones[:2] + twos[:1] + ones[2:4] + twos[1:] + ones[4:], level=1),  # (chr2 between)
               bf.write_bigwig(str(tmp_path / "c.bw"), chroms, ones[:4], buf_size=0)]  # (stored)
    wanted = [(bigwig.open_bigwig(r["path"]), "chr1") for r in records]
    table, spans, blocks, file_first, n_out = bigwig._chrom_layout(wanted, "device")
    leaves = [bf.expected_leaves(r, "chr1") for r in records]
    assert [len(v) for v in leaves] == [3, 5, 4] and file_first.tolist() == [0, 3, 8, 12]
    assert blocks == [(k, index, offset) for k, v in enumerate(leaves) for index, (offset, _) in enumerate(v)]
    runs = []  # (file, first byte, size): the blocks of a file, merged where one begins exactly where the one before ends
    for k, v in enumerate(leaves):
        for offset, size in v:
            if runs and runs[-1][0] == k and runs[-1][1] + runs[-1][2] == offset:
                runs[-1][2] += size
            else:
                runs.append([k, offset, size])
    assert [k for k, _, _ in runs] == [0, 1, 1, 1, 2]  # (a.bw one run; b.bw cut twice by a chr2 block; c.bw one run, not merged with b.bw's)
    assert [tuple(s[1:]) for s in spans.spans] == [(offset, size) for _, offset, size in runs]
    files = [open(r["path"], "rb").read() for r in records]
    sizes = [size for v in leaves for _, size in v]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    capacity = [r["uncompressBufSize"] or max(size for _, size in v) for r, v in zip(records, leaves)]
    assert table[:, 0].tolist() == starts[:-1].tolist() and table[:, 1].tolist() == starts[1:].tolist() and spans.n_comp == starts[-1]
    assert table[:, 2].tolist() == [capacity[k] for k, _, _ in blocks] and table[:, 4].tolist() == [0] * 8 + [1] * 4
    strides = [(c + 7) // 8 * 8 for c in table[:, 2].tolist()]
    assert table[:, 3].tolist() == np.concatenate([[0], np.cumsum(strides[:-1])]).tolist() and n_out == sum(strides)
    up_table, comp = uploaded(table, spans)
    assert np.array_equal(up_table, table)
    assert comp == b"".join(files[k][offset: offset + size] for k, v in enumerate(leaves) for offset, size in v)
    bigwig.clear_bigwig_cache()


def test_no_blocks_at_all(tmp_path):
    from rocco_amd import bam, bigwig, inflate

    table, spans, owner, slices = bam._group_layout([stream(memoryview(b""), [], 0, 0)])
    assert table.shape == (0, 5) and spans.spans == [] and spans.n_comp == 0 and owner == [] and slices == [(0, 0)]
    up_table, comp = uploaded(table, spans)
    assert up_table.shape == (0, 5) and comp == b""
    assert [t.numel() for t in inflate.upload_blocks(bam.bgzf_block_table([]), [], 0, "cpu")] == [0, 0]
    record = bf.write_bigwig(str(tmp_path / "empty.bw"), [("chr1", 1000), ("chr2", 1000)], bf.fixed_sections(1, 1, 5, seed=1))
    table, spans, blocks, file_first, n_out = bigwig._chrom_layout([(bigwig.open_bigwig(record["path"]), "chr1")], "device")
    assert table.shape == (0, 5) and spans.spans == [] and blocks == [] and file_first.tolist() == [0, 0] and n_out == 0
    bigwig.clear_bigwig_cache()
