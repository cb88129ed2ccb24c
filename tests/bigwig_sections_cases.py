"""(not a test module) The inputs the section decode (rocco_amd/csrc/bigwig_sections.h: the kernels of bigwig_sections.hip and their host
twin) is held against on the CPU, on the GPU and in tests/tools/bigwig_sections_san.cpp: the inflated sections of every file of
`bigwig_files.valid_cases()` and of bigwig_score_cases.py laid out as `inflate_chrom_blocks` lays them out, hand-built sections one per
refusal, and what the second reader of bigwig_files.py expects of them.  Run as a script it writes them as `.case` files:

    python tests/bigwig_sections_cases.py DIR"""
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (HERE, os.path.dirname(HERE)) if p not in sys.path]

import bigwig_files as bf  # noqa: E402
import bigwig_score_cases as sc  # noqa: E402

ERR_TABLE, ERR_SHORT, ERR_TYPE, ERR_ITEMS, ERR_WRAP = 4, 8, 9, 10, 11  # include/rocco_hip.h
COLUMNS = 5
POISON = 0xA5


def widened_bits(bits32: np.ndarray) -> np.ndarray:
    """The float64 bit patterns C's (double) makes of float32 bit patterns (NumPy's astype is that conversion)."""
    with np.errstate(invalid="ignore"):  # (a signalling NaN raises the flag as it gets its quiet bit)
        return np.ascontiguousarray(bits32, dtype=np.uint32).view(np.float32).astype(np.float64).view(np.uint64)


def layout(sections, capacity=None, tight=True, poison=True):
    """(slots, table int64 [n][5], produced int64 [n]) for raw section bytes, as `inflate_chrom_blocks` lays them out: one slot per
    section, the stride the capacity rounded up to 8.  `capacity`: None for the longest section.  The bytes of a slot behind
    `produced` are POISON (no result may depend on them); with `tight` the buffer ends where the last slot's capacity ends."""
    capacity = max((len(s) for s in sections), default=0) if capacity is None else capacity
    stride = (capacity + 7) // 8 * 8
    n = len(sections)
    table = np.zeros((n, COLUMNS), dtype=np.int64)
    table[:, 2], table[:, 3] = capacity, stride * np.arange(n, dtype=np.int64)
    size = (stride * (n - 1) + capacity if tight else stride * n) if n else 0
    slots = np.full(size, POISON if poison else 0, dtype=np.uint8)
    for k, s in enumerate(sections):
        slots[stride * k: stride * k + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return slots, table, np.asarray([len(s) for s in sections], dtype=np.int64)


def file_sections(path, record, chromosome):
    """The inflated sections of the chromosome's data blocks in R-tree leaf order, by `zlib.decompress`."""
    with open(path, "rb") as handle:
        raw = handle.read()
    stored = record["uncompressBufSize"] == 0
    return [raw[o: o + n] if stored else zlib.decompress(raw[o: o + n]) for o, n in bf.expected_leaves(record, chromosome)]


def file_inputs(written):
    """[(label, sections, chromosome id, chromosome length, expected (starts, ends, float32 bits))] for [(label, path, record,
    chromosomes)]: one entry per chromosome the file has."""
    out = []
    for label, path, record, chromosomes in written:
        for chromosome in chromosomes:
            if chromosome not in record["chroms"]:
                continue
            tid, length = record["chroms"][chromosome]
            out.append((f"{label}: {chromosome}", file_sections(path, record, chromosome), tid, length,
                        bf.as_arrays(bf.expected_intervals(path, chromosome))))
    return out


def write_all(directory):
    """Writes the files of both case lists into `directory`: [(label, path, the writer's record, the chromosomes to ask for)]."""
    written = []
    for index, case in enumerate(bf.valid_cases()):
        path, record = bf.write_case(case, directory, index)
        written.append((case[0], path, record, case[4]))
    for name, (chroms, sections, how) in sc.files().items():
        path = os.path.join(str(directory), name)
        written.append((name, path, bf.write_bigwig(path, chroms, sections, **how), [c for c, _ in chroms]))
    return written


def census(inputs) -> dict:
    """What the inputs make the decode do, counted from the sections' own bytes by the second reader's rules."""
    seen = {"types": set(), "skipped": 0, "dropped_at_end": 0, "all_dropped": 0, "counts": set(), "trailing": 0}
    for _, sections, tid, length, _ in inputs:
        for data in sections:
            chrom, first, _, step, span, kind, _, count = struct.unpack_from("<IIIIIBBH", data, 0)
            if chrom != tid:
                seen["skipped"] += 1
                continue
            seen["types"].add(kind)
            seen["counts"].add(count)
            size = {1: 12, 2: 8, 3: 4}[kind]
            seen["trailing"] += len(data) > 24 + count * size
            starts = [struct.unpack_from("<I", data, 24 + size * j)[0] if kind < 3 else first + j * step for j in range(count)]
            dropped = sum(s >= length for s in starts)
            seen["dropped_at_end"] += dropped
            seen["all_dropped"] += count > 0 and dropped == count
    return seen


def header(chrom=0, start=0, end=0, step=0, span=0, kind=3, count=0) -> bytes:
    return struct.pack("<IIIIIBBH", chrom, start, end, step, span, kind, 0, count)


def refusals():
    """[(label, the section's bytes, the status it must get)]: one hand-built section per refusal, chromosome id 0."""
    floats = bf.f32([1, 2, 3]).tobytes()
    return [
        ("23 bytes", header(count=0)[:23], ERR_SHORT),
        ("no byte at all", b"", ERR_SHORT),
        ("type 0", header(kind=0, count=1, step=50, span=50) + floats, ERR_TYPE),
        ("type 4", header(kind=4, count=1, step=50, span=50) + floats, ERR_TYPE),
        ("fixedStep: itemCount one more than fits", header(kind=3, count=4, step=50, span=50) + floats, ERR_ITEMS),
        ("variableStep: itemCount one more than fits", header(kind=2, count=2, span=50) + struct.pack("<If", 10, 1.0) + b"\0" * 7, ERR_ITEMS),
        ("bedGraph: itemCount one more than fits", header(kind=1, count=2) + struct.pack("<IIf", 10, 20, 1.0) + b"\0" * 11, ERR_ITEMS),
        ("the header's maximum of items over 24 bytes", header(kind=3, count=65535, step=1, span=1), ERR_ITEMS),
        ("variableStep: start + span = 2^32", header(kind=2, count=2, span=16) + struct.pack("<IfIf", 100, 1.0, 2 ** 32 - 16, 2.0), ERR_WRAP),
        ("fixedStep: start + span = 2^32 in its last item", header(kind=3, start=2 ** 32 - 150, count=3, step=50, span=50) + floats, ERR_WRAP),
    ]


def accepted_edges():
    """[(label, the section's bytes, chromosome length, expected [(start, end, value)])]: hand-built sections at the edge of a rule."""
    top = 2 ** 32 - 1
    return [
        ("the header alone", header(count=0), 1000, []),
        ("fixedStep: an end of exactly 2^32 - 1", header(kind=3, start=top - 100, count=2, step=50, span=50) + bf.f32([1, 2]).tobytes(), top,
         [(top - 100, top - 50, 1.0), (top - 50, top, 2.0)]),
        ("bedGraph: an end of 0 and a start at the length", header(kind=1, count=3) + struct.pack("<IIfIIfIIf", 0, 0, 1.0, 5, 9, 2.0, 1000, 1001, 3.0),
         1000, [(5, 9, 2.0)]),
        ("a skipped block of type 9 and an impossible count", header(chrom=7, kind=9, count=65535), 1000, []),
        ("a NaN with a payload, a signalling NaN, -0.0, a subnormal", header(kind=3, count=4, step=10, span=10) +
         np.asarray([0x7FC12345, 0xFF800001, 0x80000000, 0x00000003], dtype=np.uint32).tobytes(), 1000, None),
    ]


def write_case_file(path, slots, table, produced, file_first, ids, lengths, status, expected):
    starts, ends, bits = expected if expected is not None else (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint32))
    with open(path, "wb") as handle:
        handle.write(np.asarray([slots.size, table.shape[0], len(ids), starts.size], dtype=np.int64).tobytes())
        for a, dtype in ((slots, np.uint8), (table, np.int64), (produced, np.int64), (file_first, np.int64), (ids, np.int64), (lengths, np.int64),
                         (status, np.int32), (starts, np.int64), (ends, np.int64), (widened_bits(bits), np.uint64)):
            handle.write(np.ascontiguousarray(a, dtype=dtype).tobytes())


def write_case_files(directory, work) -> int:
    """The `.case` files of tests/tools/bigwig_sections_san.cpp in `directory` (the bigWig files themselves go to `work`)."""
    n = 0
    for label, sections, tid, length, expected in file_inputs(write_all(work)):
        slots, table, produced = layout(sections)
        write_case_file(os.path.join(str(directory), f"file{n:03d}.case"), slots, table, produced, [0, len(sections)], [tid], [length],
                        np.zeros(len(sections), dtype=np.int32), expected)
        n += 1
    good = bf.section_bytes(bf.fixed_sections(0, 1, 3, seed=1)[0])
    for label, data, want in refusals():  # (alone at its exact size, and between two sound sections)
        for sections, status in (([data], [want]), ([good, data, good], [0, want, 0])):
            slots, table, produced = layout(sections, capacity=len(data) if len(sections) == 1 else None)
            write_case_file(os.path.join(str(directory), f"refusal{n:03d}.case"), slots, table, produced, [0, len(sections)], [0], [10 ** 7],
                            np.asarray(status, dtype=np.int32), None)
            n += 1
    for label, data, length, want in accepted_edges():
        if want is None:
            continue
        slots, table, produced = layout([data])
        write_case_file(os.path.join(str(directory), f"edge{n:03d}.case"), slots, table, produced, [0, 1], [0], [length], np.zeros(1, dtype=np.int32),
                        bf.as_arrays(want))
        n += 1
    return n


if __name__ == "__main__":
    import pathlib
    import tempfile

    target = pathlib.Path(sys.argv[1])
    target.mkdir(parents=True, exist_ok=True)
    with tempfile.TemporaryDirectory() as work:
        print(f"wrote {write_case_files(target, pathlib.Path(work))} case files to {target}")
