"""The bigWig files the reader of rocco_amd/bigwig.py and the zlib-framed inflate of csrc/bgzf_inflate.hip are held against (note (31)).  Pure Python: a writer of complete files
(`write_bigwig`: header, zoom headers, total summary, chromosome B+ tree of one or several levels, data sections of the three
types each compressed on its own or stored, an R-tree of one or several levels, zoom levels of junk), a second reader that
shares no code with the package (`expected_intervals`: `struct`, `zlib.decompress` and sequential loops, libBigWig's rules as
the format and its documentation state them), the case lists, and the expected verdict of a block, which is zlib's."""
import struct
import zlib

import numpy as np

import bgzf_expected as gx

MAGIC, CHROM_MAGIC, RTREE_MAGIC = 0x888FFC26, 0x78CA8C91, 0x2468ACE0
MAX_U32 = 0xFFFFFFFF

# the status words of include/rocco_hip.h
ERR_STREAM, ERR_LENGTH, ERR_TABLE, ERR_HEADER, ERR_ADLER, ERR_TRUNCATED = 1, 2, 4, 5, 6, 7
HEADER_REASONS = {"incorrect header check": 1, "unknown compression method": 2, "invalid window size": 3, "dictionary": 4}


# ---- the writer ----------------------------------------------------------------------------------------------------------------
def f32(values):
    return np.asarray(values, dtype=np.float32)


def section(chrom, kind, items, start=0, step=0, span=0, **how):
    """A data section: `kind` 1 (items (start, end, value)), 2 ((start, value), with `span`) or 3 ((value), with `start`, `step`,
    `span`).  `how`: header_chrom, header_type, item_count (what the 24-byte header says where it differs), leaf (the R-tree
    leaf's (startChrom, startBase, endChrom, endBase) where it differs), payload (the block on disk as it is), pad (junk bytes
    behind the stream, inside the leaf's dataSize)."""
    return dict(chrom=chrom, type=kind, items=list(items), start=start, step=step, span=span, **how)


def section_extent(sec):
    """(chromStart, chromEnd) of a section's header."""
    items, kind = sec["items"], sec["type"]
    if kind == 1:
        return (min(i[0] for i in items), max(i[1] for i in items)) if items else (0, 0)
    if kind == 2:
        return (min(i[0] for i in items), max(i[0] for i in items) + sec["span"]) if items else (0, 0)
    return sec["start"], sec["start"] + max(len(items) - 1, 0) * sec["step"] + sec["span"]


def section_bytes(sec) -> bytes:
    """The uncompressed bytes of a section: the 24-byte header and the items."""
    items, kind = sec["items"], sec["type"]
    first, last = section_extent(sec)
    head = struct.pack("<IIIIIBBH", sec.get("header_chrom", sec["chrom"]), first & MAX_U32, min(last, MAX_U32), sec["step"], sec["span"],
                       sec.get("header_type", kind), 0, sec.get("item_count", len(items)))
    if kind == 1:
        body = b"".join(struct.pack("<II", s, e) + f32(v).tobytes() for s, e, v in items)
    elif kind == 2:
        body = b"".join(struct.pack("<I", s) + f32(v).tobytes() for s, v in items)
    else:
        body = f32(items).tobytes()
    return head + body


def zlib_stream(data: bytes, level) -> bytes:
    if level == "fixed":
        packer = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
        return packer.compress(data) + packer.flush()
    return zlib.compress(data, level)


def _tree(entries, fan, base, pack_leaf, pack_child, bounds):
    """A tree over `entries` with up to `fan` items per node, the root at `base`, children behind their parents level by
    level.  Returns (bytes, [(offset, is_leaf, count)] root first)."""
    levels = [[entries[i: i + fan] for i in range(0, len(entries), fan)] or [[]]]
    while len(levels[0]) > 1:
        below = levels[0]
        levels.insert(0, [list(range(i, min(i + fan, len(below)))) for i in range(0, len(below), fan)])
    leaf_size, child_size = len(pack_leaf(entries[0])) if entries else 0, len(pack_child(bounds([entries[0]]) if entries else None, 0)) if entries else 0
    offsets, at = [], base
    for depth, nodes in enumerate(levels):
        size = leaf_size if depth == len(levels) - 1 else child_size
        offsets.append([])
        for node in nodes:
            offsets[-1].append(at)
            at += 4 + len(node) * size
    cover = [None] * len(levels)  # per level, per node: the bounds of everything below it
    cover[-1] = [bounds(node) if node else None for node in levels[-1]]
    for depth in range(len(levels) - 2, -1, -1):
        cover[depth] = [bounds_of_bounds([cover[depth + 1][c] for c in node]) for node in levels[depth]]
    out, nodes_out = [], []
    for depth, nodes in enumerate(levels):
        is_leaf = depth == len(levels) - 1
        for k, node in enumerate(nodes):
            nodes_out.append((offsets[depth][k], is_leaf, len(node)))
            out.append(struct.pack("<BBH", 1 if is_leaf else 0, 0, len(node)))
            for item in node:
                out.append(pack_leaf(item) if is_leaf else pack_child(cover[depth + 1][item], offsets[depth + 1][item]))
    return b"".join(out), nodes_out


def bounds_of_bounds(covers):
    covers = [c for c in covers if c is not None]
    return min(c[0] for c in covers), max(c[1] for c in covers)


def write_bigwig(path, chroms, sections, *, buf_size=None, level=6, items_per_slot=1024, block_size=256, zooms=0, key_size=None,
                 chrom_block_size=None):
    """Writes a complete bigWig file.  `chroms`: [(name, length)], a chromosome's id is its index; `sections`: `section()`
    dicts in file order; `buf_size`: None for exactly the largest section, 0 for a stored file; `level`: 0 .. 9 or "fixed".
    Returns the writer's own record of what it wrote: header fields, {name: (id, length)}, per section (dataOffset, dataSize),
    the nodes of both trees."""
    names = [name.encode("latin-1") for name, _ in chroms]
    key_size = max(len(n) for n in names) if key_size is None else key_size
    assert all(len(n) <= key_size for n in names)
    raws = [section_bytes(sec) for sec in sections]
    if buf_size is None:
        buf_size = max((len(r) for r in raws), default=0)
    disk = [sec["payload"] if "payload" in sec else ((raw if buf_size == 0 else zlib_stream(raw, level)) + bytes([0xEE]) * sec.get("pad", 0))
            for sec, raw in zip(sections, raws)]
    header_at, zoom_at = 0, 64
    summary_at = zoom_at + 24 * zooms
    chrom_at = summary_at + 40
    entries = [(names[k], k, length) for k, (_, length) in enumerate(chroms)]
    chrom_tree, chrom_nodes = _tree(
        entries, chrom_block_size or max(len(entries), 1), chrom_at + 32, lambda e: e[0].ljust(key_size, b"\0") + struct.pack("<II", e[1], e[2]),
        lambda cover, child: (cover[0] if cover else b"").ljust(key_size, b"\0") + struct.pack("<Q", child), lambda node: (node[0][0], node[-1][0]))
    chrom_head = struct.pack("<IIIIQQ", CHROM_MAGIC, chrom_block_size or max(len(entries), 1), key_size, 8, len(entries), 0)
    data_at = chrom_at + 32 + len(chrom_tree)
    blocks, at = [], data_at + 8
    for payload in disk:
        blocks.append((at, len(payload)))
        at += len(payload)
    index_at = at
    leaves = []
    for sec, (offset, size) in zip(sections, blocks):
        first, last = section_extent(sec)
        leaves.append(tuple(sec.get("leaf", (sec["chrom"], first, sec["chrom"], min(last, MAX_U32)))) + (offset, size))
    rtree, rtree_nodes = _tree(
        leaves, block_size, index_at + 48, lambda e: struct.pack("<IIIIQQ", *e),
        lambda cover, child: struct.pack("<IIIIQ", *(cover[0] + cover[1] if cover else (0, 0, 0, 0)), child),
        lambda node: (min((e[0], e[1]) for e in node), max((e[2], e[3]) for e in node)))
    whole = (min((e[0], e[1]) for e in leaves), max((e[2], e[3]) for e in leaves)) if leaves else ((0, 0), (0, 0))
    rtree_head = struct.pack("<IIQIIIIQII", RTREE_MAGIC, block_size, len(leaves), *whole[0], *whole[1], index_at, items_per_slot, 0)
    zoom_data_at = index_at + 48 + len(rtree)
    junk = np.random.default_rng(77).integers(0, 256, size=200, dtype=np.uint8).tobytes()
    zoom_headers = b"".join(struct.pack("<IIQQ", 10 * 4 ** k, 0, zoom_data_at + 200 * k, zoom_data_at + 200 * k + 100) for k in range(zooms))
    values = np.concatenate([f32([i[-1] for i in sec["items"]] if sec["type"] < 3 else sec["items"]).astype(np.float64) for sec in sections] or
                            [np.zeros(0)])
    finite = values[np.isfinite(values)]
    summary = struct.pack("<Qdddd", finite.size, float(finite.min()) if finite.size else 0.0, float(finite.max()) if finite.size else 0.0,
                          float(finite.sum()), float((finite * finite).sum()))
    header = struct.pack("<IHHQQQHHQQIQ", MAGIC, 4, zooms, chrom_at, data_at, index_at, 0, 0, 0, summary_at, buf_size, 0)
    body = header + zoom_headers + summary + chrom_head + chrom_tree + struct.pack("<Q", len(sections)) + b"".join(disk) + rtree_head + rtree + \
        junk * zooms + struct.pack("<I", MAGIC)
    assert len(header) == 64 and len(summary) == 40 and len(chrom_head) == 32 and len(rtree_head) == 48
    with open(path, "wb") as handle:
        handle.write(body)
    return dict(path=str(path), size=len(body), version=4, zoomLevels=zooms, chromosomeTreeOffset=chrom_at, fullDataOffset=data_at,
                fullIndexOffset=index_at, totalSummaryOffset=summary_at, uncompressBufSize=buf_size,
                chroms={name: (k, length) for k, (name, length) in enumerate(chroms)}, blocks=blocks, leaves=leaves, rtree_nodes=rtree_nodes,
                chrom_nodes=chrom_nodes, sections=sections, raws=raws, disk=disk, zoom_data=(zoom_data_at, 200 * zooms))


def expected_leaves(record, chromosome):
    """The (dataOffset, dataSize) a correct reader collects for the chromosome: the leaves that overlap [0, length), in order."""
    tid, length = record["chroms"][chromosome]
    return [(leaf[4], leaf[5]) for leaf in record["leaves"] if _leaf_overlaps(leaf, tid, 0, length)]


# ---- the second reader ----------------------------------------------------------------------------------------------------------
def _leaf_overlaps(item, tid, start, end):
    sc, sb, ec, eb = item[:4]
    if tid < sc or tid > ec:
        return False
    if sc != ec:
        if tid == sc:
            return not sb >= end
        if tid == ec:
            return not eb <= start
        return True
    return not (sb >= end or eb <= start)


def expected_intervals(path, chromosome):
    """What pyBigWig's `intervals(chromosome)` returns by libBigWig's rules: [(start, end, value as np.float32)], or None for
    a chromosome the file does not have.  An end beyond 2**32 - 1 raises OverflowError (libBigWig would wrap)."""
    with open(path, "rb") as handle:
        raw = handle.read()
    magic, _, zoom_levels, chrom_at, _, index_at, _, _, _, _, buf_size, _ = struct.unpack_from("<IHHQQQHHQQIQ", raw, 0)
    assert magic == MAGIC
    cmagic, _, key_size, _, _, _ = struct.unpack_from("<IIIIQQ", raw, chrom_at)
    assert cmagic == CHROM_MAGIC
    found = []

    def find(node):
        is_leaf, _, count = struct.unpack_from("<BBH", raw, node)
        for k in range(count):
            at = node + 4 + k * (key_size + 8)
            if is_leaf:
                if raw[at: at + key_size].rstrip(b"\0") == chromosome.encode("latin-1"):
                    found.append(struct.unpack_from("<II", raw, at + key_size))
            else:
                find(struct.unpack_from("<Q", raw, at + key_size)[0])

    find(chrom_at + 32)
    if not found:
        return None
    tid, length = found[0]
    assert struct.unpack_from("<I", raw, index_at)[0] == RTREE_MAGIC
    blocks = []

    def collect(node):
        is_leaf, _, count = struct.unpack_from("<BBH", raw, node)
        for k in range(count):
            if is_leaf:
                item = struct.unpack_from("<IIIIQQ", raw, node + 4 + 32 * k)
                if _leaf_overlaps(item, tid, 0, length):
                    blocks.append((item[4], item[5]))
            else:
                item = struct.unpack_from("<IIIIQ", raw, node + 4 + 24 * k)
                if _leaf_overlaps(item, tid, 0, length):
                    collect(item[4])

    collect(index_at + 48)
    out = []
    for offset, size in blocks:
        data = raw[offset: offset + size]
        if buf_size > 0:
            data = zlib.decompress(data)
        chrom, first, _, step, span, kind, _, count = struct.unpack_from("<IIIIIBBH", data, 0)
        if chrom != tid:
            continue
        for j in range(count):
            if kind == 1:
                start, end = struct.unpack_from("<II", data, 24 + 12 * j)
                value = np.frombuffer(data, dtype="<f4", count=1, offset=24 + 12 * j + 8)[0]
            elif kind == 2:
                (start,) = struct.unpack_from("<I", data, 24 + 8 * j)
                end = start + span
                value = np.frombuffer(data, dtype="<f4", count=1, offset=24 + 8 * j + 4)[0]
            else:
                assert kind == 3
                start = first + j * step
                end = start + span
                value = np.frombuffer(data, dtype="<f4", count=1, offset=24 + 4 * j)[0]
            if end > MAX_U32:
                raise OverflowError("libBigWig would wrap around")
            if end <= 0 or start >= length:
                continue
            out.append((start, end, value))
    return out


def intervals_of_sections(sections, tid, length):
    """The same rules over the writer's input (no file): [(start, end, float32)] of the sections whose R-tree leaf overlaps
    [0, length) of `tid` and whose header names `tid`."""
    out = []
    for sec in sections:
        first, last = section_extent(sec)
        leaf = sec.get("leaf", (sec["chrom"], first, sec["chrom"], min(last, MAX_U32)))
        if not _leaf_overlaps(leaf, tid, 0, length) or sec.get("header_chrom", sec["chrom"]) != tid:
            continue
        for j, item in enumerate(sec["items"]):
            if sec["type"] == 1:
                start, end, value = item
            elif sec["type"] == 2:
                start, end, value = item[0], item[0] + sec["span"], item[1]
            else:
                start = sec["start"] + j * sec["step"]
                end, value = start + sec["span"], item
            if not (end <= 0 or start >= length):
                out.append((start, end, np.float32(value)))
    return out


def as_arrays(intervals):
    """(starts int64, ends int64, the float32 values' bit patterns as uint32)."""
    starts = np.asarray([i[0] for i in intervals], dtype=np.int64)
    ends = np.asarray([i[1] for i in intervals], dtype=np.int64)
    return starts, ends, f32([i[2] for i in intervals]).view(np.uint32)


# ---- the valid files -------------------------------------------------------------------------------------------------------------
def fixed_sections(chrom, n_sections, per, first=0, step=50, span=50, seed=0, gap_every=0):
    """`n_sections` fixedStep sections of `per` items each, one behind the other; a gap of 3 bins behind every `gap_every`-th."""
    rng = np.random.default_rng(seed)
    out, at = [], first
    for k in range(n_sections):
        out.append(section(chrom, 3, f32(rng.random(per) * 10), start=at, step=step, span=span))
        at += per * step + (3 * step if gap_every and (k + 1) % gap_every == 0 else 0)
    return out


def var_sections(chrom, n_sections, per, first=0, step=50, span=50, seed=0):
    rng = np.random.default_rng(seed)
    out, at = [], first
    for _ in range(n_sections):
        out.append(section(chrom, 2, [(at + j * step, np.float32(v)) for j, v in enumerate(rng.random(per) * 10)], span=span))
        at += per * step
    return out


def bed_sections(chrom, n_sections, per, first=0, step=50, seed=0):
    rng = np.random.default_rng(seed)
    out, at = [], first
    for _ in range(n_sections):
        out.append(section(chrom, 1, [(at + j * step, at + (j + 1) * step, np.float32(v)) for j, v in enumerate(rng.random(per) * 10)]))
        at += per * step
    return out


MAKERS = {1: bed_sections, 2: var_sections, 3: fixed_sections}


def valid_cases():
    """[(label, chroms, sections, keywords of `write_bigwig`, the chromosomes to ask for)]."""
    big = 10 ** 7
    one = [("chr1", big)]
    cases = []
    for kind, name in ((1, "bedGraph"), (2, "variableStep"), (3, "fixedStep")):
        for per in (1, 2, 1024):
            cases.append((f"{name}, one section of {per} items", one, MAKERS[kind](0, 1, per, seed=per), {}, ["chr1"]))
        cases.append((f"{name}, 300 sections of 7 items", one, MAKERS[kind](0, 300, 7, seed=3), dict(block_size=16), ["chr1"]))
    mixed = bed_sections(0, 2, 5, first=0, seed=1) + var_sections(0, 2, 5, first=500, seed=2) + fixed_sections(0, 2, 5, first=1000, seed=3)
    cases.append(("the three types mixed in one chromosome", one, mixed, {}, ["chr1"]))
    for level in (0, 1, 6, 9, "fixed"):
        cases.append((f"level {level}", one, fixed_sections(0, 3, 400, seed=9), dict(level=level), ["chr1"]))
    cases.append(("buf_size 65536", one, fixed_sections(0, 3, 100, seed=4), dict(buf_size=65536), ["chr1"]))
    cases.append(("a stored file", one, mixed, dict(buf_size=0), ["chr1"]))
    forty = [(f"chr{k}", 5000 + 100 * k) for k in range(40)]
    spread = [s for k in range(40) if k != 17 for s in fixed_sections(k, 1, 4, first=100 * (k % 3), seed=k)]
    cases.append(("40 chromosomes: the first, the last, one with no section, one absent", forty, spread,
                  dict(chrom_block_size=4, key_size=32, block_size=4), ["chr0", "chr39", "chr17", "chr21", "chrNone"]))
    cases.append(("a key size of 1", [("1", 3000), ("2", 3000)], fixed_sections(0, 1, 3) + fixed_sections(1, 2, 3, seed=5), dict(key_size=1), ["1", "2"]))
    other = fixed_sections(0, 1, 5, seed=6) + [section(0, 3, f32([1, 2, 3]), start=250, step=50, span=50, header_chrom=1)] + \
        fixed_sections(0, 1, 5, first=400, seed=7)
    cases.append(("a leaf whose section names another chromosome", [("chrA", 9000), ("chrB", 9000)], other, {}, ["chrA", "chrB"]))
    edge = [section(0, 1, [(900, 950, 1.5), (950, 1000, 2.5), (1000, 1050, 3.5), (1050, 1100, 4.5)]),
            section(0, 3, f32([5, 6, 7]), start=1100, step=50, span=50, leaf=(0, 0, 0, 1000)),
            section(0, 2, [(850, 8.0), (1000, 9.0)], span=50, leaf=(0, 0, 0, 1000))]
    cases.append(("items at and beyond the chromosome's length", [("chrE", 1000)], edge, {}, ["chrE"]))
    cases.append(("gaps, so that the dense fill writes zeros", one, fixed_sections(0, 6, 9, seed=8, gap_every=2), {}, ["chr1"]))
    cases.append(("an R-tree of depth 3 with block_size 2", one, fixed_sections(0, 7, 3, seed=10), dict(block_size=2), ["chr1"]))
    cases.append(("zoom levels of junk, junk behind every stream", one, [dict(s, pad=5) for s in var_sections(0, 3, 6, seed=11)], dict(zooms=3), ["chr1"]))
    return cases


def write_case(case, directory, index=0):
    """Writes a case's file; returns (path, the writer's record)."""
    label, chroms, sections, how, _ = case
    path = str(directory / f"case{index}.bw")
    return path, write_bigwig(path, chroms, sections, **how)


# ---- zlib streams: valid, corrupt, mutated -----------------------------------------------------------------------------------------
def expected_status(span: bytes, capacity: int, framing: int = 0):
    """(the status word `rocco_hip_zlib_inflate` must give, the bytes where it accepts): zlib.decompress raises -> the class
    and zlib's words; more than `capacity` bytes -> _LENGTH; else the bytes.  Precedence: header, stream, truncated, length,
    Adler-32 (so a stream that is too long AND fails its Adler-32, which zlib reports, is a length error: its bytes are not kept)."""
    if framing == 1:
        return (ERR_LENGTH, None) if len(span) > capacity else (0, bytes(span))
    try:
        data = zlib.decompress(span)
    except zlib.error as exc:
        text = str(exc)
        if text.startswith("Error 2 "):
            return ERR_HEADER | HEADER_REASONS["dictionary"] << 8, None
        words = text[text.index("data: ") + 6:]
        if words in HEADER_REASONS:
            return ERR_HEADER | HEADER_REASONS[words] << 8, None
        if words == "incorrect data check":
            return (ERR_LENGTH if len(zlib.decompress(span[2:], wbits=-15)) > capacity else ERR_ADLER), None
        if words == "incomplete or truncated stream":
            if len(span) < 2 or span[1] & 0x20:
                return ERR_TRUNCATED, None
            body = zlib.decompressobj(wbits=-15)
            body.decompress(span[2:])
            return (ERR_TRUNCATED if body.eof else ERR_STREAM | 12 << 8), None
        from rocco_amd import bam

        number = {said: why for why, said in bam._STREAM_REASON_TEXT.items()}
        assert words == gx.stream_reason(span[2:]), (words, "the raw stream fails for another reason")
        return ERR_STREAM | number[words] << 8, None
    return (ERR_LENGTH, None) if len(data) > capacity else (0, data)


def status_class(status: int) -> str:
    return {0: "accepted", ERR_STREAM: "stream", ERR_LENGTH: "length", ERR_TABLE: "table", ERR_HEADER: "header", ERR_ADLER: "adler",
            ERR_TRUNCATED: "truncated"}[status & 0xFF]


def payloads():
    """The uncompressed sections the stream lists are made of."""
    return [section_bytes(s) for s in bed_sections(0, 1, 40, seed=21) + var_sections(0, 1, 300, seed=22) + fixed_sections(0, 1, 1024, seed=23) +
            fixed_sections(0, 1, 1, seed=24) + bed_sections(0, 1, 5000, seed=25)]


def valid_streams():
    """[(label, span, capacity, framing)] that must be accepted."""
    out = []
    for k, data in enumerate(payloads()):
        for level in (0, 1, 6, 9, "fixed"):
            out.append((f"payload {k}, level {level}", zlib_stream(data, level), len(data) if k % 2 else 65536, 0))
        out.append((f"payload {k}, junk behind the Adler-32", zlib_stream(data, 6) + b"\x00\xff\x17", len(data), 0))
        if len(data) <= 65536:
            out.append((f"payload {k}, stored as it is", data, len(data), 1))
    for cinfo in range(8):  # (every window size of the header; zlib's compressor writes 7)
        cmf = cinfo << 4 | 8
        body = zlib.compress(payloads()[0], 6)
        out.append((f"CINFO {cinfo}", bytes([cmf, _fcheck(cmf)]) + body[2:], 65536, 0))
    out.append(("an empty payload", zlib.compress(b""), 0, 0))
    out.append(("an empty stored span", b"", 0, 1))
    for label, cdata, data in gx.hand_streams()[1:]:
        out.append((f"hand-assembled: {label}", b"\x78\x9c" + cdata + struct.pack(">I", zlib.adler32(data)), len(data), 0))
    return out


def corrupt_streams():
    """[(label, span, capacity, framing, the class of the status it must get)]: one per acceptance rule."""
    data = payloads()[1]
    good = zlib_stream(data, 6)
    n = len(data)
    out = [("incorrect header check", bytes([good[0], good[1] ^ 1]) + good[2:], n, 0, "header"),
           ("unknown compression method", bytes([0x79, _fcheck(0x79)]) + good[2:], n, 0, "header"),
           ("invalid window size", bytes([0x88, _fcheck(0x88)]) + good[2:], n, 0, "header"),
           ("FDICT set", bytes([0x78, _fcheck(0x78, 0x20)]) + b"\0\0\0\1" + good[2:], n, 0, "header"),
           ("FDICT set and no room for the dictionary id", bytes([0x78, _fcheck(0x78, 0x20)]) + b"\0\0", n, 0, "truncated"),
           ("one header byte", good[:1], n, 0, "truncated"),
           ("an empty span", b"", n, 0, "truncated"),
           ("the header alone", good[:2], n, 0, "stream"),
           ("Adler-32 off by one bit", good[:-1] + bytes([good[-1] ^ 0x04]), n, 0, "adler"),
           ("Adler-32 off in its first byte", good[:-4] + bytes([good[-4] ^ 0x80]) + good[-3:], n, 0, "adler"),
           ("a stream cut inside the Adler-32: 3 of 4 bytes", good[:-1], n, 0, "truncated"),
           ("a stream cut inside the Adler-32: 0 of 4 bytes", good[:-4], n, 0, "truncated"),
           ("a stream cut inside the deflate data", good[:-9], n, 0, "stream"),
           ("inflates to capacity + 1", good, n - 1, 0, "length"),
           ("inflates to capacity + 1 and fails its Adler-32", good[:-1] + bytes([good[-1] ^ 1]), n - 1, 0, "length"),
           ("a stored span of capacity + 1", data, n - 1, 1, "length"),
           ("capacity 0 under a match", zlib.compress(b"ab" * 700), 0, 0, "length"),
           ("one payload bit flipped under a stored deflate block", _flip(zlib_stream(data, 0), 700, 0x10), n, 0, "adler")]
    for label, bad, _ in gx.corrupt_blocks():  # (every stream reason of the shared decoder, under zlib framing)
        _, lo, hi, _, _ = gx.blocks_of(bad)[0]
        cdata = bad[lo:hi]
        if expected_status(b"\x78\x9c" + cdata + b"\0\0\0\1", 65536)[0] & 0xFF == ERR_STREAM:
            out.append((f"deflate data: {label}", b"\x78\x9c" + cdata + b"\0\0\0\1", 65536, 0, "stream"))
    return out


def _fcheck(cmf: int, flags: int = 0x80) -> int:
    flg = flags & 0xE0
    return flg | (31 - (cmf * 256 + flg) % 31) % 31


def _flip(data: bytes, at: int, mask: int) -> bytes:
    return data[:at] + bytes([data[at] ^ mask]) + data[at + 1:]


MUTATIONS = 1500
_mutations = None


def mutation_bases():
    """The compressed spans of three small files: (span, capacity); the third file keeps junk behind every stream."""
    bases = []
    for k, (maker, level, pad) in enumerate(((bed_sections, 6, 0), (var_sections, 0, 0), (fixed_sections, "fixed", 12))):
        for sec in maker(0, 4, 6 + k, seed=30 + k):
            raw = section_bytes(sec)
            bases.append((zlib_stream(raw, level) + bytes([0xEE]) * pad, len(raw)))
    return bases


def mutated_streams():
    """[(span, capacity)]: MUTATIONS seeded single-byte mutations (a bit flipped or a byte replaced) of `mutation_bases()`."""
    global _mutations
    if _mutations is None:
        rng = np.random.default_rng(2031)
        bases = mutation_bases()
        _mutations = []
        for _ in range(MUTATIONS):
            span, capacity = bases[int(rng.integers(0, len(bases)))]
            changed = bytearray(span)
            at = int(rng.integers(0, len(changed)))
            if rng.random() < 0.5:
                changed[at] ^= 1 << int(rng.integers(0, 8))
            else:
                changed[at] = (changed[at] + int(rng.integers(1, 256))) & 0xFF
            _mutations.append((bytes(changed), capacity))
    return _mutations


GUARD, GUARD_BYTE = 24, 0xA5


def table_of(streams, guard=GUARD):
    """(the compressed buffer, the block table int64 [n][5], the size of the output buffer) for [(span, capacity, framing)]:
    slots of the capacity rounded up to 8 with `guard` bytes in front of, between and behind them."""
    comp, rows, at, slot = [], [], 0, guard
    for span, capacity, framing in streams:
        rows.append((at, at + len(span), capacity, slot, framing))
        comp.append(span)
        at += len(span)
        slot += (capacity + 7) // 8 * 8 + guard
    return b"".join(comp), np.asarray(rows, dtype=np.int64).reshape(-1, 5), slot


def verify(streams, table, status, produced, out, label=""):
    """`status`, `produced` and `out` (filled with GUARD_BYTE before the call) against `expected_status` of every stream: the
    status word whole (class and reason), the bytes and their number where zlib accepts, and not one byte changed outside
    the slots' capacities.  Returns the index of the first refused block or -1."""
    inside = np.zeros(out.shape[0], dtype=bool)
    first = -1
    for k, (span, capacity, framing) in enumerate(streams):
        want, data = expected_status(span, capacity, framing)
        slot = int(table[k, 3])
        inside[slot: slot + capacity] = True
        assert int(status[k]) == want, (label, k, int(status[k]), want)
        if want == 0:
            assert int(produced[k]) == len(data) and out[slot: slot + len(data)].tobytes() == data, (label, k)
        elif first < 0:
            first = k
        if want == ERR_LENGTH:
            assert int(produced[k]) == (len(span) if framing else len(zlib.decompress(span[2:], wbits=-15))), (label, k)
    assert np.all(out[~inside] == GUARD_BYTE), (label, "a byte outside the slots was written")
    return first
