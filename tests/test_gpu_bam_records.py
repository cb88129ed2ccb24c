"""GPU: the record walk and the record fields of csrc/bam_records.hip over the inflated bytes of
the fixtures of tests/golden/bam_files.npz and over streams built here: the offsets against the sequential walk of
tests/bam_expected.py, the eight arrays and the contig offsets against htslib's own dump, bit for bit and whatever the
segment size, the guesses or the slab size; every corruption an ordinary ValueError that names the record and its offset."""
import struct

import numpy as np
import pytest

import bam_expected as bx

pytestmark = pytest.mark.gpu

FILES = ["mixed", "blocks", "longread", "header_only", "one_record", "unplaced_only", "cg", "decoy"]
N_REF = 3
_streams = {}


def stream(key):
    """(inflated bytes, first record, sequential offsets) of a fixture, computed once."""
    if key not in _streams:
        data, _ = bx.inflate(bx.bam_bytes(key))
        entry0 = bx.header(data)[2]
        _streams[key] = (data, entry0, bx.walk(data, entry0)[0])
    return _streams[key]


def upload(gpu, data):
    import torch

    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).to(gpu)


def host(fields):
    out = {}
    for name, dtype in bx.FIELDS:
        a = fields[name].cpu().numpy()
        out[name] = a.view(np.uint16) if name == "flag" else a
        assert out[name].dtype == dtype
    return out


@pytest.mark.parametrize("segment_bytes", [64, 256, 4096, None])
@pytest.mark.parametrize("key", FILES)
def test_walk_and_fields_equal_htslib_at_every_segment_size(gpu, key, segment_bytes):
    from rocco_amd import bam

    data, entry0, want_offsets = stream(key)
    bytes_t = upload(gpu, data)
    offsets, report = bam.walk_records_device(bytes_t, entry0, N_REF, segment_bytes, want_segment_entries=True)
    S = segment_bytes or bx.DEFAULT_SEGMENT_BYTES
    assert report["error"] == 0 and report["error_offset"] == -1 and report["end_offset"] == len(data)
    assert report["records"] == want_offsets.size and report["segments"] == max((len(data) + S - 1) // S, 1)
    assert offsets.dtype.is_floating_point is False and np.array_equal(offsets.cpu().numpy(), want_offsets)
    assert np.array_equal(report["segment_entries"].cpu().numpy(), bx.true_entries(data, entry0, S))
    assert report["wrong_guesses"] == bx.wrong_guesses(data, entry0, N_REF, S) == report["repair_rounds"] + int(np.count_nonzero(
        (bx.guesses(data, entry0, N_REF, S) >= 0) & (bx.true_entries(data, entry0, S) < 0)))
    if segment_bytes is None and key != "decoy":
        assert report["wrong_guesses"] == 0 and report["repair_rounds"] == 0
    fields, firsts, (code, record) = bam.record_fields_device(bytes_t, offsets, N_REF)
    want = bx.dump(key)
    got = host(fields)
    if key == "cg":
        cg = int(np.flatnonzero(want["qlen"] == 33000)[0])
        assert (code, record) == (bx.ERR_CG_TAG, cg)
        with pytest.raises(ValueError, match=rf"record {cg} at byte {want_offsets[cg]} of the inflated stream: .*CG tag"):
            bam.decode_records_device(bytes_t, entry0, N_REF, segment_bytes, name="cg.bam")
        keep = np.arange(want_offsets.size) != cg
    else:
        assert (code, record) == (0, -1)
        keep = np.ones(want_offsets.size, dtype=bool)
    for name, _ in bx.FIELDS:
        mask = keep if name in ("end", "qlen") else slice(None)
        assert np.array_equal(got[name][mask], want[name][mask]), name
    assert firsts == bx.contig_first(want["tid"], N_REF).tolist()


@pytest.mark.parametrize("key", ["mixed", "blocks", "longread", "decoy"])
def test_guess_mode_zero_leaves_the_work_to_the_repair(gpu, key):
    from rocco_amd import bam

    data, entry0, want_offsets = stream(key)
    bytes_t = upload(gpu, data)
    for S in (64, 4096):
        offsets, report = bam.walk_records_device(bytes_t, entry0, N_REF, S, guess_mode=0, want_segment_entries=True)
        truth = bx.true_entries(data, entry0, S)
        assert np.array_equal(offsets.cpu().numpy(), want_offsets) and report["error"] == 0
        assert np.array_equal(report["segment_entries"].cpu().numpy(), truth)
        seg0 = entry0 // S
        starts_on_boundary = int(np.count_nonzero(truth[seg0 + 1:] == (np.arange(seg0 + 1, truth.size) * S)))
        with_start = int(np.count_nonzero(truth[seg0 + 1:] >= 0))
        assert report["repair_rounds"] == with_start - starts_on_boundary and report["repair_rounds"] > 0.9 * with_start
        # (every segment behind entry0's up to the one of the last record's start guessed its first byte; behind the chain's
        # end there is no truth left to guess wrongly)
        assert report["wrong_guesses"] == int(want_offsets[-1]) // S - seg0 - starts_on_boundary


def test_decoy_fools_the_guess_not_the_result(gpu):
    from rocco_amd import bam

    _, meta = bx.golden()
    data, entry0, want_offsets = stream("decoy")
    S, at = meta["decoy_segment_bytes"], meta["decoy_offset"]
    assert bx.guesses(data, entry0, N_REF, S)[at // S] == at
    offsets, report = bam.walk_records_device(upload(gpu, data), entry0, N_REF, S, want_segment_entries=True)
    assert report["wrong_guesses"] >= 1 and report["error"] == 0
    assert np.array_equal(offsets.cpu().numpy(), want_offsets)
    assert int(report["segment_entries"][at // S]) != at


@pytest.mark.parametrize("segment_bytes", [64, 256])
def test_segments_under_the_long_read_are_empty(gpu, segment_bytes):
    from rocco_amd import bam

    data, entry0, want_offsets = stream("longread")
    sizes = np.diff(np.concatenate([want_offsets, [len(data)]]))
    k = int(np.argmax(sizes))
    lo, hi = int(want_offsets[k]), int(want_offsets[k] + sizes[k])
    assert sizes[k] > 4500
    _, report = bam.walk_records_device(upload(gpu, data), entry0, N_REF, segment_bytes, want_segment_entries=True)
    entries = report["segment_entries"].cpu().numpy()
    covered = np.arange(lo // segment_bytes + 1, hi // segment_bytes)
    assert covered.size >= 4500 // segment_bytes - 2 and np.all(entries[covered] == -1)
    assert entries[lo // segment_bytes] in (lo, *want_offsets[want_offsets // segment_bytes == lo // segment_bytes].tolist())


def test_synthetic_stream_seams(gpu):
    """Records of chosen lengths, S = 64: a block_size word across a segment boundary (a start at 64 k - 2), a record ending
    exactly at a segment's end, one longer than several segments, and the last ending exactly at the slab's end; the same
    stream cut one byte short ends in a truncated record that the report places."""
    from rocco_amd import bam

    header = bx.make_header([("a", 1000), ("b", 1000)])  # 12 + 2 * 10 = 32 bytes
    assert len(header) == 32
    lengths = [94, 42, 88, 64, 42, 300, 42, 96]  # starts: 32, 126 (= 128 - 2), 168, 256, 320, 362, 662, 704; end: 800
    records = [bx.make_record(n, tid=0 if k < 5 else 1, pos=10 * k, cigar=((0, 20),), l_seq=0) for k, n in enumerate(lengths)]
    data = header + b"".join(records)
    want = np.cumsum([32] + lengths)[:-1]
    assert want[1] == 126 and want[3] == 256 and len(data) == 800 and np.array_equal(bx.walk(data, 32)[0], want)
    for S in (64, 128, 256):
        for mode in (1, 0):
            offsets, report = bam.walk_records_device(upload(gpu, data), 32, 2, S, guess_mode=mode, want_segment_entries=True)
            assert np.array_equal(offsets.cpu().numpy(), want) and report["error"] == 0 and report["end_offset"] == 800
            assert np.array_equal(report["segment_entries"].cpu().numpy(), bx.true_entries(data, 32, S))
    fields, firsts, (code, _) = bam.record_fields_device(upload(gpu, data), offsets, 2)
    assert code == 0 and firsts == [0, 5, 8, 8] and host(fields)["end"].tolist() == [10 * k + 20 for k in range(8)]
    offsets, report = bam.walk_records_device(upload(gpu, data[:-1]), 32, 2, 64)
    assert np.array_equal(offsets.cpu().numpy(), want[:-1])
    assert (report["error"], report["error_offset"], report["end_offset"]) == (bx.ERR_TRUNCATED, 704, 704)
    offsets, report = bam.walk_records_device(upload(gpu, data[:706]), 32, 2, 64)  # (half a block_size word)
    assert offsets.shape[0] == 7 and (report["error"], report["error_offset"]) == (bx.ERR_TRUNCATED, 704)
    offsets, report = bam.walk_records_device(upload(gpu, header), 32, 2, 64)
    assert offsets.shape[0] == 0 and report["error"] == 0 and report["end_offset"] == 32


@pytest.mark.parametrize("slab_bytes", [1000, 4096])
@pytest.mark.parametrize("key", ["blocks", "mixed", "longread"])
def test_slabs_give_the_single_slab_result(gpu, tmp_path, key, slab_bytes):
    from rocco_amd import bam

    if key != "blocks":  # (htslib's own blocks hold 64 KiB: cut them again, so that the slabs are as small as asked)
        data, _, _ = stream(key)
        path = str(tmp_path / f"{key}.bam")
        with open(path, "wb") as handle:
            handle.write(bx.bgzf_compress(data, cuts=range(777, len(data), 777)))
    else:
        path = bx.write_bam(tmp_path, key)
    whole_report, slab_report = {}, {}
    whole, unplaced_whole = bam.read_alignment_file(path, device=gpu, report=whole_report)
    slabs, unplaced_slabs = bam.read_alignment_file(path, device=gpu, slab_bytes=slab_bytes, report=slab_report)
    want = bx.dump(key)
    assert whole_report["slabs"] == 1 and slab_report["slabs"] > 3
    assert unplaced_whole == unplaced_slabs == int((want["tid"] == -1).sum())
    assert whole.name == slabs.name == path and whole.contigs == slabs.contigs == [("chrB", 120000), ("chrA", 400000), ("chrC", 90000)]
    for k, (contig, _) in enumerate(whole.contigs):
        on = want["tid"] == k
        for name, _ in bx.FIELDS[1:]:
            for file in (whole, slabs):
                a = getattr(file.records[contig], name).cpu().numpy()
                assert np.array_equal(a.view(np.uint16) if name == "flag" else a, want[name][on]), (contig, name)


def corrupt(data, at, fmt, value):
    out = bytearray(data)
    struct.pack_into(fmt, out, at, value)
    return bytes(out)


def test_corruptions_are_ordinary_errors(gpu, tmp_path):
    """Each corruption, written into a copy of the inflated bytes, raises a ValueError that names the record and its byte
    offset; the process stays healthy (the intact stream decodes afterwards)."""
    import torch

    from rocco_amd import bam

    data, entry0, offsets = stream("mixed")
    want = bx.dump("mixed")
    r = 700
    p = int(offsets[r])
    assert want["tid"][r] >= 0 and want["tid"][r] == want["tid"][r + 1]
    mapped_with_seq = next(int(k) for k in range(100, offsets.size) if not want["flag"][k] & 4 and struct.unpack_from("<i", data, int(offsets[k]) + 20)[0] > 0
                           and struct.unpack_from("<H", data, int(offsets[k]) + 16)[0] > 0)
    q = int(offsets[mapped_with_seq])
    first_b, first_a = int(np.flatnonzero(want["tid"] == 0)[0]), int(np.flatnonzero(want["tid"] == 1)[0])
    swapped = bytearray(data)
    for k in range(first_b, first_a):
        struct.pack_into("<i", swapped, int(offsets[k]) + 4, 1)
    for k in range(first_a, int(np.flatnonzero(want["tid"] == 2)[0])):
        struct.pack_into("<i", swapped, int(offsets[k]) + 4, 0)
    cases = [
        ("block_size = 31", corrupt(data, p, "<i", 31), r, p, "block_size is below 32"),
        ("block_size past the end", corrupt(data, p, "<i", len(data)), r, p, "the stream ends inside it"),
        ("negative block_size", corrupt(data, p, "<i", -7), r, p, "block_size is below 32"),
        ("l_read_name = 0", corrupt(data, p + 12, "<B", 0), r, p, "l_read_name is 0"),
        ("sizes", corrupt(data, p + 20, "<i", 1 << 20), r, p, "do not fit its block_size"),
        ("negative l_seq", corrupt(data, p + 20, "<i", -1), r, p, "do not fit its block_size"),
        ("tid = n_ref", corrupt(data, p + 4, "<i", N_REF), r, p, "refID or next_refID"),
        ("mtid = -2", corrupt(data, p + 24, "<i", -2), r, p, "refID or next_refID"),
        ("CIGAR / l_seq", corrupt(data, q + 36 + data[q + 12], "<I", (7 << 4) | 0), mapped_with_seq, q, "differs from l_seq"),
        ("negative pos", corrupt(data, p + 8, "<i", -1), r, p, "negative position"),
        ("end beyond 2^31", corrupt(data, int(offsets[mapped_with_seq]) + 8, "<i", (1 << 31) - 10), mapped_with_seq, q, "2\\*\\*31"),
        ("contigs swapped", bytes(swapped), first_a, int(offsets[first_a]), "not coordinate-sorted"),
    ]
    assert struct.unpack_from("<I", data, q + 36 + data[q + 12])[0] != (7 << 4)
    for label, bad, record, offset, text in cases:
        for S in (64, None):
            with pytest.raises(ValueError, match=rf"bad\.bam: record {record} at byte {offset} of the inflated stream: .*{text}"):
                bam.decode_records_device(upload(gpu, bad), entry0, N_REF, S, name="bad.bam")
    fields, firsts, report = bam.decode_records_device(upload(gpu, data), entry0, N_REF, name="good.bam")
    assert report["records"] == offsets.size and np.array_equal(host(fields)["pos"], want["pos"])
    torch.cuda.synchronize()
    # an offset that frames no record: an error code, no access outside the buffer
    bogus = torch.tensor([int(offsets[0]), len(data) - 10, -5, 1 << 40], dtype=torch.int64, device=gpu)
    _, _, (code, record) = bam.record_fields_device(upload(gpu, data), bogus, N_REF)
    assert (code, record) == (bx.ERR_OFFSET, 1)
    # through the file reader: the file is named, the slab's position is added to the offset
    path = str(tmp_path / "bad.bam")
    with open(path, "wb") as handle:
        handle.write(bx.bgzf_compress(corrupt(data, p + 12, "<B", 0), cuts=range(5000, len(data), 5000)))
    for slab_bytes in (1 << 30, 6000):
        with pytest.raises(ValueError, match=rf"{path}: record {r} at byte {p} of the inflated stream: .*l_read_name is 0"):
            bam.read_alignment_file(path, device=gpu, slab_bytes=slab_bytes)
    with open(path, "wb") as handle:
        handle.write(bx.bgzf_compress(data[:-3]))
    with pytest.raises(ValueError, match=rf"{path}: record {offsets.size - 1} at byte {offsets[-1]} of the inflated stream: the stream ends inside it"):
        bam.read_alignment_file(path, device=gpu)


def test_arguments_are_checked(gpu):
    import torch

    from rocco_amd import bam

    data, entry0, _ = stream("one_record")
    bytes_t = upload(gpu, data)
    for S in (0, 32, 96, 1 << 31):
        with pytest.raises(ValueError):
            bam.walk_records_device(bytes_t, entry0, N_REF, S)
    with pytest.raises(ValueError):
        bam.walk_records_device(bytes_t, len(data) + 1, N_REF)
    with pytest.raises(ValueError):
        bam.walk_records_device(bytes_t, entry0, N_REF, guess_mode=2)
    with pytest.raises(TypeError):
        bam.walk_records_device(torch.zeros(4, dtype=torch.int32, device=gpu), 0, N_REF)
    assert bam.bam_shape() == {"guess_depth": bx.GUESS_DEPTH, "segment_bytes": bx.DEFAULT_SEGMENT_BYTES, "threads": 256}
