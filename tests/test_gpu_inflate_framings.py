"""GPU: the one kernel pair of csrc/bgzf_inflate.hip under its two framings (DESIGN.md notes (29), (31)): the same deflate
payloads as BGZF rows (`rocco_hip_bgzf_inflate`) and as zlib rows (`rocco_hip_zlib_inflate`) inflate to the same bytes; a
flipped check value is refused by the framing's own code; and the bigWig reader's K-file table costs one inflate call."""
import struct
import zlib

import numpy as np
import pytest

import bgzf_expected as gx
import bigwig_files as bf

pytestmark = pytest.mark.gpu

_payloads = None


def payloads():
    """[(label, raw deflate data, the bytes it inflates to)]: the deflate data of every block of `gx.valid_files()`, each
    distinct one once, cut where its final deflate block ends (BGZF ignores what follows inside the span; under zlib framing
    the Adler-32 follows at once)."""
    global _payloads
    if _payloads is None:
        seen, _payloads = set(), []
        for label, raw in gx.valid_files():
            for _, lo, hi, crc, isize in gx.blocks_of(raw):
                body = zlib.decompressobj(wbits=-15)
                data = body.decompress(raw[lo:hi])
                cdata = raw[lo: hi - len(body.unused_data)]
                assert body.eof and len(data) == isize and zlib.crc32(data) == crc
                if cdata not in seen:
                    seen.add(cdata)
                    _payloads.append((label, cdata, data))
    return _payloads


def bgzf_rows(items):
    """(comp, table) for [(deflate data, the bytes, the CRC32 to state)]: the spans one behind the other, no frame between."""
    rows, at, out_at = [], 0, 0
    for cdata, data, crc in items:
        rows.append((at, at + len(cdata), len(data), crc, out_at))
        at, out_at = at + len(cdata), out_at + len(data)
    return b"".join(c for c, _, _ in items), np.asarray(rows, dtype=np.int64).reshape(-1, 5)


def zlib_rows(items):
    """(comp, table) for [(deflate data, the bytes, the Adler-32 to state)]: `zlib.compress`'s header, the data, the check
    value; capacity = the bytes' length, slots at the prefix sum of the lengths (as the BGZF rows have them)."""
    spans = [zlib.compress(b"")[:2] + cdata + struct.pack(">I", adler) for cdata, _, adler in items]
    rows, at, out_at = [], 0, 0
    for span, (_, data, _) in zip(spans, items):
        rows.append((at, at + len(span), len(data), out_at, 0))
        at, out_at = at + len(span), out_at + len(data)
    return b"".join(spans), np.asarray(rows, dtype=np.int64).reshape(-1, 5)


def on_device(gpu, comp, table, n_out, framing):
    import torch

    from rocco_amd import bam, bigwig

    comp_t = torch.from_numpy(np.frombuffer(comp, dtype=np.uint8).copy()).to(gpu)
    out = torch.full((n_out,), 0xA5, dtype=torch.uint8, device=gpu)
    if framing == "bgzf":
        status, report = bam.inflate_blocks_device(comp_t, torch.from_numpy(table).to(gpu), out, want_status=True)
        produced = None
    else:
        status, produced, report = bigwig.zlib_inflate_blocks_device(comp_t, torch.from_numpy(table).to(gpu), out)
        produced = produced.cpu().numpy()
    return status.cpu().numpy(), produced, report, out.cpu().numpy()


def test_the_same_payloads_under_both_framings_give_the_same_bytes(gpu):
    items = payloads()
    assert len(items) > 600 and {0, 1, 65280, 65536} <= {len(data) for _, _, data in items}
    whole = b"".join(data for _, _, data in items)
    comp, table = bgzf_rows([(cdata, data, zlib.crc32(data)) for _, cdata, data in items])
    status, _, report, as_bgzf = on_device(gpu, comp, table, len(whole), "bgzf")
    assert not status.any() and report == {"block": -1, "status": 0, "produced": 0}
    comp, table = zlib_rows([(cdata, data, zlib.adler32(data)) for _, cdata, data in items])
    status, produced, report, as_zlib = on_device(gpu, comp, table, len(whole), "zlib")
    assert not status.any() and report == {"block": -1, "status": 0, "produced": 0}
    assert produced.tolist() == [len(data) for _, _, data in items]  # (produced == ISIZE)
    assert as_bgzf.tobytes() == whole and as_zlib.tobytes() == whole


def thirteen():
    """Thirteen payloads of every kind: empty, around one wavefront's lanes, the largest, stored, fixed, dynamic, flushed,
    hand-assembled."""
    first = {}
    for label, cdata, data in payloads():
        first.setdefault(label, (cdata, data))
    labels = ["0 random bytes", "1 random bytes", "63 random bytes", "64 random bytes", "65 random bytes", "65280 random bytes",
              "65536 bytes of one value", "level 0, text", "level 6, records", "Z_FIXED, text", "Z_RLE, 65536 zeros",
              "Z_SYNC_FLUSH between deflate blocks, records"]
    hand = next(label for label in first if label.startswith("hand-assembled"))
    return [first[label] for label in labels + [hand]]


@pytest.mark.parametrize("framing", ["bgzf", "zlib"])
def test_a_flipped_check_value_is_refused_by_the_framings_own_code(gpu, framing):
    """26 rows: each of 13 streams as it is, then with one bit of its stated check value flipped (another bit for every stream)."""
    streams = thirteen()
    assert len(streams) == 13
    check, rows, code = (zlib.crc32, bgzf_rows, gx.ERR_CRC) if framing == "bgzf" else (zlib.adler32, zlib_rows, bf.ERR_ADLER)
    items = []
    for k, (cdata, data) in enumerate(streams):
        items += [(cdata, data, check(data)), (cdata, data, check(data) ^ (1 << (k * 5 % 32)))]
    comp, table = rows(items)
    n_out = sum(len(data) for _, data, _ in items)
    status, produced, report, out = on_device(gpu, comp, table, n_out, framing)
    assert status.tolist() == [0, code] * 13
    assert report == {"block": 1, "status": code, "produced": len(streams[0][1])}
    if produced is not None:
        assert produced.tolist() == [len(data) for _, data, _ in items]
    starts = np.concatenate([[0], np.cumsum([len(data) for _, data, _ in items])]).tolist()
    assert all(out[starts[k]: starts[k + 1]].tobytes() == items[k][1] for k in range(0, 26, 2))


def test_three_bigwig_files_cost_one_inflate_call(gpu, tmp_path, monkeypatch):
    from rocco_amd import bigwig

    bigwig.clear_bigwig_cache()
    records = [bf.write_bigwig(str(tmp_path / f"{k}.bw"), [("chr1", 10 ** 6)], bf.fixed_sections(0, 3 + k, 40, seed=50 + k), level=level)
               for k, level in enumerate((6, 0, "fixed"))]
    calls = []
    real = bigwig.zlib_inflate_blocks_device
    monkeypatch.setattr(bigwig, "zlib_inflate_blocks_device", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    wanted = [(bigwig.open_bigwig(r["path"]), "chr1") for r in records]
    slots, table, produced, first = bigwig.inflate_chrom_blocks(wanted, gpu, "device")
    assert calls == [1] and first.tolist() == [0, 3, 7, 12]
    slots, table, produced = slots.cpu().numpy(), table.cpu().numpy(), produced.cpu().numpy()
    want = [raw for r in records for raw in r["raws"]]
    assert produced.tolist() == [len(raw) for raw in want]
    assert all(slots[int(table[k, 3]): int(table[k, 3]) + len(raw)].tobytes() == raw for k, raw in enumerate(want))
    bigwig.clear_bigwig_cache()
