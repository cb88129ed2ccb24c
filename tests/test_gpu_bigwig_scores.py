"""GPU: the reference's `get_bigwig_chrom_scores` and `generate_chrom_matrix` over bigWig paths with no pyBigWig (DESIGN.md section 0
row f10, note (31); rocco_amd/bigwig.py) against tests/golden/bigwig_scores.npz / .json, which the REFERENCE's own functions wrote
(tests/golden/make_golden_bigwig_scores.py) over the same files: intervals equal, values and matrices by bit pattern, exception types and
texts equal, WARNING records in order -- after the digest of every file written again here is checked.  And the binding of INTEGRATION.md:
`run_chromosomes` over bigWig paths writes the BED bytes it writes through the pyBigWig route of rocco_amd.readtracks."""
import json
import logging
import os
import types

import numpy as np
import pytest

import bigwig_files as bf
import bigwig_score_cases as sc
from assemble_golden import FakeBigWig

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERRORS = {"ValueError": ValueError, "FileNotFoundError": FileNotFoundError, "RuntimeError": RuntimeError}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "bigwig_scores.json"), "r", encoding="utf-8") as handle:
        return np.load(os.path.join(GOLDEN, "bigwig_scores.npz")), json.load(handle)


@pytest.fixture(scope="module")
def files(tmp_path_factory, golden):
    """The files written again; none is used before its digest is the stored one."""
    directory = tmp_path_factory.mktemp("bigwig_scores")
    paths = sc.write_files(directory)
    specs = sc.files()
    assert set(golden[1]["files"]) == set(specs)
    for name, (chroms, _, _) in specs.items():
        assert sc.digest(paths[name], chroms) == golden[1]["files"][name], name
    return directory, paths


def held_against(record, arrays, key, directory, caplog, call, to_host):
    """Runs `call`; its return value, its exception and its WARNING records against what the reference did."""
    where = str(directory)
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        if "error" in record:
            with pytest.raises(ERRORS[record["error"]["type"]]) as info:
                call()
            assert type(info.value) is ERRORS[record["error"]["type"]] and str(info.value) == record["error"]["text"].replace("{dir}", where), record["name"]
        else:
            intervals, values = to_host(*call())
            if record.get("none"):
                assert intervals is None and values is None, record["name"]
            else:
                want_i, want_v = arrays[f"{key}_intervals"], arrays[f"{key}_values"]
                assert np.array_equal(intervals, want_i) and str(intervals.dtype) == record["intervals_dtype"], record["name"]
                assert values.shape == want_v.shape and str(values.dtype) == record["values_dtype"], record["name"]
                assert np.array_equal(values.view(np.uint64 if values.dtype == np.float64 else np.uint32),
                                      want_v.view(np.uint64 if want_v.dtype == np.float64 else np.uint32)), record["name"]
    log = [[r.levelname, r.getMessage()] for r in caplog.records if r.levelno >= logging.WARNING and r.name.startswith("rocco_amd")]
    assert log == [[level, text.replace("{dir}", where)] for level, text in record["log"]], record["name"]


def test_get_bigwig_chrom_scores_against_the_reference(gpu, golden, files, caplog):
    from rocco_amd import bigwig

    arrays, meta = golden
    directory, paths = files
    assert [r["name"] for r in meta["scores"]] == [c[0] for c in sc.score_cases()]
    for index, ((name, file, chromosome, sizes, kwargs), record) in enumerate(zip(sc.score_cases(), meta["scores"])):
        args = (sc.path_of(paths, directory, file), chromosome, sc.path_of(paths, directory, sizes))
        held_against(record, arrays, f"s{index}", directory, caplog, lambda: bigwig.get_bigwig_chrom_scores(*args, **kwargs), lambda i, v: (i, v))
        if "error" not in record:  # the device form: the same track left in HBM
            first, step, full = bigwig.get_bigwig_chrom_scores_device(*args, **kwargs, inflate="host")
            if record.get("none"):
                assert first is None and step is None and full is None
            else:
                want_i = arrays[f"s{index}_intervals"]
                assert first == want_i[0] and full.is_cuda and (want_i.size == 1 or step == want_i[1] - want_i[0])
                assert np.array_equal(full.cpu().numpy().view(np.uint64), arrays[f"s{index}_values"].view(np.uint64)), name


def test_generate_chrom_matrix_against_the_reference(gpu, golden, files, caplog):
    from rocco_amd import bigwig

    arrays, meta = golden
    directory, paths = files
    assert [r["name"] for r in meta["matrix"]] == [c[0] for c in sc.matrix_cases()]

    def device_to_host(starts, matrix):
        assert matrix is None or matrix.is_cuda
        return starts, None if matrix is None else matrix.cpu().numpy()

    for index, ((name, names, chromosome, kwargs), record) in enumerate(zip(sc.matrix_cases(), meta["matrix"])):
        args = (chromosome, [sc.path_of(paths, directory, f) for f in names], paths[sc.SIZES_FILE], 50)
        held_against(record, arrays, f"m{index}", directory, caplog, lambda: bigwig.generate_chrom_matrix(*args, num_processors=1, **kwargs),
                     lambda i, v: (i, v))
        held_against(record, arrays, f"m{index}", directory, caplog, lambda: bigwig.generate_chrom_matrix_device(*args, **kwargs), device_to_host)


def test_run_chromosomes_from_bigwig_paths_writes_the_same_bed(gpu, tmp_path, monkeypatch):
    """rocco_amd.readtracks.get_bigwig_chrom_scores = rocco_amd.bigwig.get_bigwig_chrom_scores and rocco_amd.rocco.generate_chrom_matrix =
    rocco_amd.bigwig.generate_chrom_matrix_device: from three bigWig paths to the combined BED with no pyBigWig, byte for
    byte what run_chromosomes writes today through rocco_amd.readtracks.generate_chrom_matrix, whose pyBigWig here is a stand-in that
    serves the second reader's intervals.  Two chromosomes, K = 3."""
    from rocco_amd import bigwig
    from rocco_amd import readtracks as rt
    from rocco_amd import rocco as impl

    chroms = [("chrP", 400000), ("chrQ", 300000)]
    rng = np.random.default_rng(2031)
    paths = []
    for k in range(3):
        sections = []
        for tid, (_, length) in enumerate(chroms):
            n = 3000 - 400 * tid
            signal = np.round(rng.gamma(1.0, 0.3, size=n), 3)
            for p in range(200, n - 100, 500):
                signal[p: p + int(rng.integers(5, 40))] += rng.gamma(6.0, 0.8) * (rng.random() < 0.9)
            first = 1000 + 50 * k  # (ragged ends: every file starts and ends elsewhere)
            for lo in range(0, n, 1024):
                part = bf.f32(signal[lo: lo + 1024])
                sections.append(bf.section(tid, 3, part, start=first + 50 * lo, step=50, span=50))
        paths.append(str(tmp_path / f"track{k}.bw"))
        bf.write_bigwig(paths[-1], chroms, sections)
    sizes = str(tmp_path / "pq.sizes")
    with open(sizes, "w", encoding="utf-8") as handle:
        handle.write("".join(f"{c}\t{n}\n" for c, n in chroms))

    def stand_in_open(path):
        listed = {c: [(int(s), int(e), float(v)) for s, e, v in bf.expected_intervals(path, c)] or None for c, _ in chroms}
        return FakeBigWig(dict(chroms), listed)

    stand_in = types.ModuleType("pyBigWig")
    stand_in.open = stand_in_open
    args = {"chrom_sizes_file": sizes, "step": 50, "round_digits": 5, "effective_genome_size": -1, "norm_method": "RPGC", "min_mapping_score": 10,
            "flag_include": None, "flag_exclude": 3844, "extend_reads": -1, "center_reads": False, "ignore_for_norm": None, "scale_factor": 1.0,
            "score_lower_bound_z": 1.0, "score_prior_df": 6.0, "score_min_effect": None, "score_precision_floor_ratio": 0.01, "gamma": None,
            "budget": None, "scale_chrom_budgets": 1.0, "budget_posterior_quantile": 0.01, "selection_penalty": None, "min_length_bp": 100,
            "narrowPeak": False, "low_memory": False, "input_track_type": "bigwig", "budget_null_draws": 6, "threads": 1}
    names = [c for c, _ in chroms]
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(rt, "pyBigWig", stand_in)
    monkeypatch.setattr(impl, "generate_chrom_matrix", rt.generate_chrom_matrix)  # today's route: pyBigWig hands over the intervals
    want = impl.run_chromosomes(names, paths, dict(args, output=str(tmp_path / "want.bed")), run_id="1")
    monkeypatch.setattr(rt, "pyBigWig", None)  # (nothing below may ask for it)
    monkeypatch.setattr(rt, "get_bigwig_chrom_scores", bigwig.get_bigwig_chrom_scores)
    through_readtracks = impl.run_chromosomes(names, paths, dict(args, output=str(tmp_path / "mid.bed")), run_id="2")
    monkeypatch.setattr(impl, "generate_chrom_matrix", bigwig.generate_chrom_matrix_device)
    got = impl.run_chromosomes(names, paths, dict(args, output=str(tmp_path / "got.bed")), run_id="3")
    with open(want, "rb") as a, open(through_readtracks, "rb") as b, open(got, "rb") as c:
        want_bytes, mid_bytes, got_bytes = a.read(), b.read(), c.read()
    assert want_bytes.count(b"\n") >= 4 and b"chrP" in want_bytes and b"chrQ" in want_bytes
    assert mid_bytes == want_bytes and got_bytes == want_bytes
