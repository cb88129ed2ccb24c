"""GPU: `rocco_amd.bigwig.read_bigwig_blocks` end to end (note (31)): the inflated data blocks of
every valid file of tests/bigwig_files.py, in R-tree leaf order, against the sections the writer compressed -- in both
inflate modes and for K files in one table --; corrupt files, which both modes refuse by the same block with the same words;
and the cache, which follows a file's mtime."""
import os
import re
import zlib

import numpy as np
import pytest

import bigwig_files as bf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    directory = tmp_path_factory.mktemp("bigwig_blocks")
    return [(case,) + bf.write_case(case, directory, k) for k, case in enumerate(bf.valid_cases())]


def wanted_blocks(record, chromosome):
    at = {block: raw for block, raw in zip(record["blocks"], record["raws"])}
    return [at[leaf] for leaf in bf.expected_leaves(record, chromosome)]


def check_blocks(slots, table, produced, want, label):
    slots, table, produced = slots.cpu().numpy(), table.cpu().numpy(), produced.cpu().numpy()
    assert table.shape == (len(want), 5) and produced.tolist() == [len(raw) for raw in want], label
    for k, raw in enumerate(want):
        slot = int(table[k, 3])
        assert slot % 8 == 0 and slots[slot: slot + len(raw)].tobytes() == raw, (label, k)


def test_blocks_of_every_valid_file_in_both_modes(gpu, written):
    import torch

    from rocco_amd import bigwig

    seen = 0
    for case, path, record in written:
        for chromosome in case[4]:
            if chromosome not in record["chroms"]:
                with pytest.raises(KeyError):
                    bigwig.read_bigwig_blocks(path, chromosome, device=gpu)
                continue
            want = wanted_blocks(record, chromosome)
            for mode in ("device", "host", None):
                slots, table, produced = bigwig.read_bigwig_blocks(path, chromosome, device=gpu, inflate=mode)
                assert slots.dtype == torch.uint8 and slots.device == gpu and table.dtype == torch.int64 and produced.dtype == torch.int64
                check_blocks(slots, table, produced, want, (case[0], chromosome, mode))
            seen += len(want)
    assert seen > 900


def test_the_blocks_of_several_files_in_one_table(gpu, written):
    from rocco_amd import bigwig

    picks = [(bigwig.open_bigwig(path), case[4][0], wanted_blocks(record, case[4][0])) for case, path, record in written
             if record["uncompressBufSize"] <= 65536]
    assert len(picks) >= 20 and any(file.header["uncompressBufSize"] == 0 for file, _, _ in picks)
    for mode in ("device", "host"):
        slots, table, produced, first = bigwig.inflate_chrom_blocks([(file, chromosome) for file, chromosome, _ in picks], gpu, mode)
        assert first.tolist() == np.concatenate([[0], np.cumsum([len(want) for _, _, want in picks])]).tolist()
        check_blocks(slots, table, produced, [raw for _, _, want in picks for raw in want], mode)


def corrupt_file(directory, name, payloads, buf_size=None):
    """A file of one chromosome whose blocks are `payloads` as they are (sound sections where an entry is None)."""
    sound = bf.fixed_sections(0, len(payloads), 20, seed=5)
    sections = [sec if payload is None else dict(sec, payload=payload) for sec, payload in zip(sound, payloads)]
    path = os.path.join(str(directory), name)
    return path, bf.write_bigwig(path, [("chr1", 10 ** 6)], sections, buf_size=buf_size, block_size=2)


def test_corrupt_files_are_refused_by_the_same_block_in_both_modes(gpu, tmp_path):
    from rocco_amd import bigwig

    raw = bf.section_bytes(bf.fixed_sections(0, 1, 20, seed=6)[0])
    good = zlib.compress(raw)
    cases = {
        "adler": ([None, good[:-1] + bytes([good[-1] ^ 2]), None], r"the zlib stream does not inflate \(incorrect data check\)"),
        "cut_in_adler": ([None, None, good[:-2]], r"the zlib stream does not inflate \(incomplete or truncated stream\)"),
        "header_check": ([bytes([good[0], good[1] ^ 1]) + good[2:], None], r"the zlib stream does not inflate \(incorrect header check\)"),
        "method": ([None, bytes([0x79, bf._fcheck(0x79)]) + good[2:]], r"the zlib stream does not inflate \(unknown compression method\)"),
        "window": ([None, bytes([0x88, bf._fcheck(0x88)]) + good[2:]], r"the zlib stream does not inflate \(invalid window size\)"),
        "dictionary": ([None, bytes([0x78, bf._fcheck(0x78, 0x20)]) + b"\0\0\0\1" + good[2:]], r"the zlib stream does not inflate \(a preset dictionary is asked for\)"),
        "stream": ([None, good[:2] + b"\x07" + good[3:]], r"the zlib stream does not inflate \(invalid block type\)"),
        "too_long": ([None, zlib.compress(raw + b"\0")],
                     r"length mismatch \(the file's uncompressBufSize is %d, the data inflates to %d\)" % (len(raw), len(raw) + 1)),
        # doubly corrupt: the first refused block in file order is named, whatever refuses the later one
        "two_bad_blocks": ([None, good[:-1] + bytes([good[-1] ^ 2]), bytes([good[0], good[1] ^ 1]) + good[2:]], r"incorrect data check"),
        "two_bad_blocks_swapped": ([None, good[:-3], good[:-1] + bytes([good[-1] ^ 2]), None], r"incomplete or truncated stream"),
    }
    for name, (payloads, words) in cases.items():
        path, record = corrupt_file(tmp_path, name + ".bw", payloads)
        index = next(k for k, p in enumerate(payloads) if p is not None)
        pattern = re.escape(f"{path}: bigWig data block {index} at file offset {record['blocks'][index][0]}: ") + ".*" + words
        said = []
        for mode in ("device", "host"):
            with pytest.raises(ValueError, match=pattern) as info:
                bigwig.read_bigwig_blocks(path, "chr1", device=gpu, inflate=mode)
            said.append(str(info.value))
        assert said[0] == said[1], name
    # a buffer size above what the device inflate holds: host mode reads the file
    big = bf.bed_sections(0, 1, 6000, seed=8)
    path = os.path.join(str(tmp_path), "big.bw")
    record = bf.write_bigwig(path, [("chr1", 10 ** 7)], big)
    with pytest.raises(ValueError, match="no CPU fallback exists for such blocks in device mode"):
        bigwig.read_bigwig_blocks(path, "chr1", device=gpu)
    check_blocks(*bigwig.read_bigwig_blocks(path, "chr1", device=gpu, inflate="host"), record["raws"], "big")


def test_the_cache_invalidates_on_mtime(gpu, tmp_path):
    from rocco_amd import bigwig

    bigwig.clear_bigwig_cache()
    path = str(tmp_path / "cached.bw")
    one, two = bf.fixed_sections(0, 2, 10, seed=1), bf.fixed_sections(0, 2, 10, seed=2)
    first = bf.write_bigwig(path, [("chr1", 10 ** 6)], one, level=0)
    check_blocks(*bigwig.read_bigwig_blocks(path, "chr1", device=gpu), first["raws"], "first")
    file = bigwig.open_bigwig(path)
    assert bigwig.open_bigwig(path) is file and file.leaves
    stat = os.stat(path)
    second = bf.write_bigwig(path, [("chr1", 10 ** 6)], two, level=0)  # (the same size: only the values differ)
    os.utime(path, ns=(stat.st_atime_ns, stat.st_mtime_ns + 10 ** 9))
    assert os.stat(path).st_size == stat.st_size and second["raws"] != first["raws"]
    check_blocks(*bigwig.read_bigwig_blocks(path, "chr1", device=gpu), second["raws"], "second")
    assert bigwig.open_bigwig(path) is not file
    bigwig.clear_bigwig_cache()
    assert not bigwig._BIGWIG_CACHE
