"""A pure-Python / NumPy statement of what the reference does with the lines of a fragments file (DESIGN.md section 0 row f13;
rocco/native/ccounts_backend.c: 359-394 the strict parser, 311-357 the barcode lookup, 2212-2346 the region count, 1583-1631
the chromosome range, 1770-1835 the mapped count, 712-772 the read length), written from the reference's C independently of
csrc/fragments_rules.h and pinned to every stored result of tests/golden/fragments.npz by tests/test_fragments_host.py.

Lines are bytes without their terminator, as htslib hands them over (``\\n`` and a ``\\r`` before it stripped)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = {"coverage": 0, "cutsite": 1, "fiveprime": 2, "center": 3}


def load_golden():
    import json

    with open(os.path.join(GOLDEN, "fragments.json"), encoding="utf-8") as handle:
        meta = json.load(handle)
    return meta, np.load(os.path.join(GOLDEN, "fragments.npz"))


def split_lines(text: bytes):
    """hts_getline's lines: split at ``\\n``, a ``\\r`` before it dropped; an unterminated last line is a line."""
    parts = text.split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    return [p[:-1] if p.endswith(b"\r") else p for p in parts]


def parse_int(field: bytes):
    """ccounts_parseInt64Field: (ok, value)."""
    if not field:
        return False, 0
    digits = field[1:] if field[:1] == b"-" else field
    if any(c < 0x30 or c > 0x39 for c in digits):
        return False, 0
    value = int(digits) if digits else 0
    return True, -value if field[:1] == b"-" else value


def c_fields(line: bytes):
    """The fields as the reference's scanners see them: a field ends at TAB, CR, LF or NUL, and the scan of the whole line
    ends at CR, LF or NUL."""
    for stop in (b"\x00", b"\r", b"\n"):
        at = line.find(stop)
        if at >= 0:
            line = line[:at]
    return line.split(b"\t")


def allowed(barcode: bytes, allow) -> bool:
    return not allow or barcode in allow


def weight_of(fields) -> int:
    ok, value = parse_int(fields[4]) if len(fields) > 4 else (False, 1)
    return value if ok and value > 0 else 1


def count_line(line: bytes, allow):
    """(start, end, weight) where the region count's loop (2212-2269) keeps the line, else the name of the rule that skips it."""
    fields = c_fields(line)
    scanned = fields[:-1] if len(fields) > 1 and fields[-1] == b"" else fields  # (a trailing TAB: the empty field behind it is never scanned)
    if line == b"" or scanned == [b""]:
        return "empty"
    start = end = 0
    for index, field in enumerate(scanned):
        if index == 1:
            ok, start = parse_int(field)
            if not ok:
                return "start"
        if index == 2:
            ok, end = parse_int(field)
            if not ok:
                return "end"
    if scanned[-1] == b"":
        return "last_empty"
    if end <= start:
        return "end_le_start"
    if len(scanned) > 3 and scanned[3] and not allowed(scanned[3], allow):
        return "barcode"
    return start, end, weight_of(scanned)


def count_region(lines, allow, r_start, r_end, step, length, mode, one_read_per_bin, census=None):
    """ccounts_countRegion's fragments branch over the non-meta lines of a contig in file order: float32 counts, the
    reference's float arithmetic in its order."""
    counts = np.zeros(length, dtype=np.float32)
    delta = np.zeros(length + 1, dtype=np.float32)

    def hit(what):
        if census is not None:
            census[what] = census.get(what, 0) + 1

    for line in lines:
        if line[:1] == b"#":
            hit("count:meta")
            continue
        kept = count_line(line, allow)
        if isinstance(kept, str):
            hit("count:" + kept)
            continue
        start, end, weight = kept
        w = np.float32(weight)
        if mode == 3 or one_read_per_bin:
            mid = (start + end) // 2
            if mid < r_start or mid >= r_end:
                hit("center:outside")
                continue
            if (mid - r_start) // step < length:
                counts[(mid - r_start) // step] += w
                hit("center:in")
            else:
                hit("center:beyond_buffer")
            continue
        if mode in (1, 2):
            for name, cut in (("cut:start", start), ("cut:end", end - 1)):
                if r_start <= cut < r_end:
                    if (cut - r_start) // step < length:
                        counts[(cut - r_start) // step] += w
                        hit(name + ":in")
                else:
                    hit(name + ":outside")
            continue
        if end <= r_start or start >= r_end:
            hit("coverage:outside")
            continue
        a, b = max(start, r_start), min(end, r_end)
        if a != start or b != end:
            hit("coverage:clipped")
        index0, index1 = (a - r_start) // step, (b - 1 - r_start) // step
        if index0 >= length:
            hit("coverage:index0_beyond")
            continue
        if index1 >= length:
            index1 = length - 1
            hit("coverage:index1_clamped")
        if index0 > index1:
            continue
        delta[index0] += w
        delta[index1 + 1] -= w
        hit("coverage:in")
    if not (mode == 3 or one_read_per_bin or mode in (1, 2)):
        running = np.float32(0.0)
        for i in range(length):
            running = np.float32(running + delta[i])
            counts[i] = np.float32(counts[i] + running)
    return counts


def three_fields(line: bytes, census=None, who=""):
    """The scan of the range and read-length loops (three fields, past the end of the line if need be): (start, end) or None."""
    fields = c_fields(line) + [b"", b""]
    ok1, start = parse_int(fields[1])
    ok2, end = parse_int(fields[2])
    rule = "start" if not ok1 else ("end" if not ok2 else ("end_le_start" if end <= start else "in"))
    if census is not None:
        census[f"{who}:{rule}"] = census.get(f"{who}:{rule}", 0) + 1
    return (start, end) if rule == "in" else None


def chrom_range(lines, census=None):
    first = last = None
    for line in lines:
        if line[:1] == b"#":
            if census is not None:
                census["range:meta"] = census.get("range:meta", 0) + 1
            continue
        found = three_fields(line, census, "range")
        if found is not None:
            first = found[0] if first is None else first
            last = found[1]
    return (0, 0) if first is None else (first, last)


def mapped_count(lines, allow, exclude, mode, one_read_per_bin, census=None):
    """ccounts_getMappedReadCount's fragments branch over ALL lines of the file (meta lines are lines)."""
    total = 0

    def hit(what):
        if census is not None:
            census[what] = census.get(what, 0) + 1

    for line in lines:
        fields = c_fields(line)
        if fields[0] in exclude:
            hit("mapped:excluded")
            continue
        if len(fields) < 5:
            hit("mapped:short")
            continue
        if fields[4] == b"":
            hit("mapped:fifth_empty")
            continue
        if fields[3] and not allowed(fields[3], allow):
            hit("mapped:barcode")
            continue
        hit("mapped:in")
        total += weight_of(fields) * (2 if mode in (1, 2) and not one_read_per_bin else 1)
    return total


def read_length(lines, min_reads=32, max_iterations=4096, census=None):
    min_reads = max(int(min_reads), 1)
    max_iterations = max(int(max_iterations), min_reads)
    lengths = []
    for line in lines:
        if len(lengths) >= max_iterations:
            break
        found = three_fields(line, census, "readlen")
        if found is None:
            continue
        lengths.append((found[1] - found[0]) & 0xFFFFFFFF)
        if len(lengths) >= min_reads:
            break
    if not lengths:
        return None
    lengths.sort()
    mid = len(lengths) // 2
    return lengths[mid] if len(lengths) % 2 else ((lengths[mid - 1] + lengths[mid]) & 0xFFFFFFFF) // 2


def parse_allowlist(raw: bytes):
    """ccounts_loadBarcodeAllowList for lines that fit its buffer: the set of entries."""
    out = set()
    for line in raw.split(b"\n"):
        token = line.lstrip(b" \t\n\v\f\r")
        if not token or token[:1] == b"#":
            continue
        out.add(token.split()[0])
    return out


def materialize(directory, meta, arrays) -> dict:
    """The stored files as files: {key: path of the .tsv.gz (its .tbi beside it)} and {"allow:<key>": path}."""
    paths = {}
    for name in arrays.files:
        if name.startswith("file_") and name.endswith("_gz"):
            key = name[5:-3]
            paths[key] = os.path.join(str(directory), key + ".tsv.gz")
            arrays[name].tofile(paths[key])
            if f"file_{key}_tbi" in arrays.files:
                arrays[f"file_{key}_tbi"].tofile(paths[key] + ".tbi")
        if name.startswith("allow_"):
            paths["allow:" + name[6:]] = os.path.join(str(directory), name + ".txt")
            arrays[name].tofile(paths["allow:" + name[6:]])
    return paths


def bgzf_block(data: bytes) -> bytes:
    import struct
    import zlib

    deflate = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = deflate.compress(data) + deflate.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25) + body +
            struct.pack("<II", zlib.crc32(data), len(data)))


def write_tbi(path: str, contigs) -> None:
    """A hand-built BED-preset ``.tbi``: ``contigs`` = [(name, (v_begin, v_end) or None)]; a contig without a span has no bin."""
    import struct

    names = b"".join(name.encode() + b"\x00" for name, _ in contigs)
    raw = b"TBI\x01" + struct.pack("<8i", len(contigs), 0x10000, 1, 2, 3, ord("#"), 0, len(names)) + names
    for _, span in contigs:
        if span is None:
            raw += struct.pack("<ii", 0, 0)
        else:
            raw += struct.pack("<iIi", 2, 0, 1) + struct.pack("<QQ", *span) + struct.pack("<Ii", 37450, 2) + struct.pack("<QQQQ", *span, 0, 0)
            raw += struct.pack("<i", 0)
    with open(path, "wb") as out:
        out.write(bgzf_block(raw) + bgzf_block(b""))


def counts_from_fields(start, end, weight, status, r_start, r_end, step, length, mode, one_read_per_bin):
    """The integer statement of the count kernels over the arrays of a field pass: (float32 counts, the largest magnitude:
    max(P, N) over the cells and every running value).  Equal to `count_region` while that magnitude stays within 2**24."""
    P, N = np.zeros(length + 1, dtype=np.int64), np.zeros(length + 1, dtype=np.int64)
    status = np.asarray(status, dtype=np.int64)
    ok = ((status & 0x1) == 0) & ((status & 0x10) != 0) & ((status & 0x20) != 0) & ((status & 0x40) == 0) & ((status & 0x400) != 0)
    s, e, w = (np.asarray(a, dtype=np.int64)[ok & (np.asarray(end) > np.asarray(start))] for a in (start, end, weight))
    if mode == 3 or one_read_per_bin:
        mid = (s + e) // 2
        keep = (mid >= r_start) & (mid < r_end) & ((mid - r_start) // step < length)
        np.add.at(P, (mid[keep] - r_start) // step, w[keep])
    elif mode in (1, 2):
        for cut in (s, e - 1):
            keep = (cut >= r_start) & (cut < r_end) & ((cut - r_start) // step < length)
            np.add.at(P, (cut[keep] - r_start) // step, w[keep])
    else:
        keep = ~((e <= r_start) | (s >= r_end))
        a, b, w = np.maximum(s[keep], r_start), np.minimum(e[keep], r_end), w[keep]
        index0, index1 = (a - r_start) // step, np.minimum((b - 1 - r_start) // step, length - 1)
        keep = (index0 < length) & (index0 <= index1)
        np.add.at(P, index0[keep], w[keep])
        np.add.at(N, index1[keep] + 1, w[keep])
        running = np.cumsum(P[:length] - N[:length])
        magnitude = max(int(P.max(initial=0)), int(N.max(initial=0)), int(np.abs(running).max(initial=0)))
        return running.astype(np.float32), magnitude
    return P[:length].astype(np.float32), int(P.max(initial=0))


def status_word(line: bytes, allow) -> dict:
    """What the status word of csrc/fragments_rules.h says of a span's line, from the statements above."""
    if line[:1] == b"#":
        return {"meta": True}
    fields = line.split(b"\t")
    scanned = fields[:-1] if len(fields) > 1 and fields[-1] == b"" else fields
    if line == b"":
        scanned = []
    ok1, start = parse_int(scanned[1]) if len(scanned) > 1 else (False, 0)
    ok2, end = parse_int(scanned[2]) if len(scanned) > 2 else (False, 0)
    okw, _ = parse_int(scanned[4]) if len(scanned) > 4 else (False, 0)
    barcode = scanned[3] if len(scanned) > 3 else b""
    return {"meta": False, "fields": min(len(scanned), 5), "start_ok": ok1, "end_ok": ok2, "start": start if ok1 else 0, "end": end if ok2 else 0,
            "last_empty": not scanned or scanned[-1] == b"", "fifth_empty": len(scanned) < 5 or scanned[4] == b"", "weight_parsed": okw,
            "weight": weight_of(scanned), "barcode_present": bool(barcode), "barcode_allowed": not barcode or allowed(barcode, allow)}
