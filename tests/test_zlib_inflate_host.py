"""CPU: the zlib-framed inflate of csrc/inflate_core.h through its host entry (rocco_hip_zlib_inflate_host: the source the
kernels of rocco_hip_zlib_inflate are compiled from, on one thread over host memory) against zlib 1.2.11 on every stream of
tests/bigwig_files.py -- bytes and `produced` equal where zlib accepts, else verdict for verdict and reason for reason -- the
census that keeps the mutation set from passing vacuously, and the BGZF host entry on a handful of its own cases: the shared
decoder still answers as before."""
import collections
import os
import re
import zlib

import numpy as np

import bgzf_expected as gx
import bigwig_files as bf


def run_host(streams, label=""):
    """The host entry over [(span, capacity, framing)] into a guarded buffer, verified; the first refused block or -1."""
    from rocco_amd import bigwig

    comp, table, n_out = bf.table_of(streams)
    out = np.full(n_out, bf.GUARD_BYTE, dtype=np.uint8)
    status, produced, report = bigwig.zlib_inflate_blocks_host(comp, table, out)
    first = bf.verify(streams, table, status, produced, out, label)
    assert report["block"] == first and report["status"] == (int(status[first]) if first >= 0 else 0), label
    if first >= 0:
        assert report["produced"] == int(produced[first]), label
    return first, status


def test_host_entry_on_the_valid_streams():
    cases = bf.valid_streams()
    assert len({label for label, *_ in cases}) == len(cases) >= 40
    for label, span, capacity, framing in cases:
        assert bf.expected_status(span, capacity, framing)[0] == 0, label
    first, _ = run_host([c[1:] for c in cases], "valid")
    assert first == -1


def test_host_entry_on_the_corrupt_streams():
    cases = bf.corrupt_streams()
    assert len({label for label, *_ in cases}) == len(cases) >= 30
    classes, header_reasons, stream_reasons = set(), set(), set()
    for label, span, capacity, framing, want in cases:
        status = bf.expected_status(span, capacity, framing)[0]
        assert bf.status_class(status) == want, (label, status)
        classes.add(want)
        if want == "header":
            header_reasons.add(status >> 8)
        if want == "stream":
            stream_reasons.add(status >> 8)
    assert classes == {"header", "stream", "truncated", "length", "adler"}
    assert header_reasons == {1, 2, 3, 4} and stream_reasons == set(range(1, 13))
    # each alone (the report names it), then all in one call (the first is reported)
    for label, span, capacity, framing, _ in cases:
        assert run_host([(span, capacity, framing)], label)[0] == 0, label
    sound = bf.valid_streams()[0][1:]
    assert run_host([sound] + [c[1:4] for c in cases] + [sound], "corrupt")[0] == 1


def test_host_entry_on_the_mutation_set_and_its_census():
    """1 500 seeded single-byte mutations of the compressed spans of three small files in one call: zlib's verdict on every
    one, none excluded.  The census is what makes this mean something: zlib alone (no code of this project) sorts at least
    50 of them into each of stream error, Adler-32 error and acceptance."""
    cases = bf.mutated_streams()
    assert len(cases) == bf.MUTATIONS == 1500
    census = collections.Counter(bf.status_class(bf.expected_status(span, capacity)[0]) for span, capacity in cases)
    assert min(census["stream"], census["adler"], census["accepted"]) >= 50, census
    assert census["header"] >= 10 and census["truncated"] + census["length"] >= 1, census
    first, status = run_host([(span, capacity, 0) for span, capacity in cases], "mutations")
    assert collections.Counter(bf.status_class(int(s)) for s in status) == census


def test_every_status_class_is_reached():
    seen = {bf.status_class(bf.expected_status(*c[1:4])[0]) for c in bf.corrupt_streams()} | {"accepted"}
    from rocco_amd import bigwig

    comp, table, n_out = bf.table_of([bf.valid_streams()[0][1:]])
    for column, value in ((0, -1), (1, len(comp) + 1), (2, 65537), (2, -1), (3, -1), (3, n_out), (4, 2), (0, int(table[0, 1]) + 1)):
        bad = table.copy()
        bad[0, column] = value
        out = np.full(n_out, bf.GUARD_BYTE, dtype=np.uint8)
        status, produced, report = bigwig.zlib_inflate_blocks_host(comp, bad, out)
        assert status[0] == bf.ERR_TABLE and report["block"] == 0 and produced[0] == 0 and np.all(out == bf.GUARD_BYTE), (column, value)
        seen.add(bf.status_class(int(status[0])))
    assert seen == {"accepted", "stream", "length", "table", "header", "adler", "truncated"}
    status, produced, report = bigwig.zlib_inflate_blocks_host(b"", np.zeros((0, 5), dtype=np.int64), np.zeros(0, dtype=np.uint8))
    assert status.size == 0 and produced.size == 0 and report["block"] == -1


def test_produced_up_to_the_capacity_is_accepted():
    data = bf.payloads()[0]
    span = zlib.compress(data)
    for capacity, want in ((len(data) - 1, bf.ERR_LENGTH), (len(data), 0), (len(data) + 1, 0), (65536, 0)):
        first, status = run_host([(span, capacity, 0)], f"capacity {capacity}")
        assert int(status[0]) == want


def test_host_mode_of_the_reader_words_a_block_as_the_status_says():
    """`rocco_amd.bigwig.host_block_status` (what inflate="host" runs per block) gives the status of `expected_status` on every
    stream of the three lists: the two modes of the reader refuse the same blocks for the same reason."""
    from rocco_amd import bigwig

    everything = [c[1:4] for c in bf.valid_streams()] + [c[1:4] for c in bf.corrupt_streams()] + [(s, c, 0) for s, c in bf.mutated_streams()]
    for k, (span, capacity, framing) in enumerate(everything):
        want, data = bf.expected_status(span, capacity, framing)
        status, got = bigwig.host_block_status(span, capacity, framing)
        assert status == want and (want != 0 or got == data), k


def test_the_bgzf_host_entry_still_answers_as_before():
    from rocco_amd import bam

    picks = [gx.valid_files()[k][1] for k in (0, 5, 12, 30)] + [raw for _, raw, _, _ in gx.corrupt_files()[:8]] + [gx.corrupt_files()[-1][1]]
    for raw in picks:
        table, n_out = gx.guarded_table(raw)
        out = np.full(n_out, gx.GUARD_BYTE, dtype=np.uint8)
        status, report = bam.inflate_blocks_host(raw, table, out)
        assert report["block"] == gx.verify(raw, table, status, out)


def test_constants_agree_with_the_c_header():
    from rocco_amd import bigwig

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "rocco_hip.h")).read()
    defined = {name: int(value) for name, value in re.findall(r"#define (ROCCO_ZLIB_[A-Z_]+) (\d+)", text)}
    assert defined == {"ROCCO_ZLIB_TABLE_COLUMNS": bigwig.ZLIB_TABLE_COLUMNS, "ROCCO_ZLIB_HEADER_REASONS": bigwig.ZLIB_HEADER_REASONS,
                       "ROCCO_ZLIB_ERR_HEADER": bigwig.ZLIB_ERR_HEADER, "ROCCO_ZLIB_ERR_ADLER": bigwig.ZLIB_ERR_ADLER,
                       "ROCCO_ZLIB_ERR_TRUNCATED": bigwig.ZLIB_ERR_TRUNCATED}
    (shift,) = re.findall(r"#define ROCCO_ZLIB_MAX_GRID \(1 << (\d+)\)", text)
    assert bigwig.ZLIB_MAX_GRID == 1 << int(shift)
    assert bigwig.zlib_shape() == {"threads": 64, "table_columns": 5, "max_capacity": 65536, "header_reasons": 4, "max_grid": bigwig.ZLIB_MAX_GRID}
    assert (bigwig.ZLIB_ERR_HEADER, bigwig.ZLIB_ERR_ADLER, bigwig.ZLIB_ERR_TRUNCATED) == (bf.ERR_HEADER, bf.ERR_ADLER, bf.ERR_TRUNCATED)
    assert sorted(bigwig._HEADER_REASON_TEXT) == [1, 2, 3, 4] and bigwig.DEFAULT_INFLATE == "device"
