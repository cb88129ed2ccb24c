"""Row f6 composed on the GPU: from decoded records to the reference's count-matrix TSV, its per-bin null values and its
narrowPeak file, byte for byte, for the scenario the reference's own raw_count_matrix / get_ecdf / multi_ecdf /
score_peaks ran (tests/golden/make_golden_interval_counts.py: `_hts_counts` and `pysam` replaced by stand-ins over the
reference's compiled counter)."""
import numpy as np
import pytest

import interval_counts_expected as iv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenario(gpu, tmp_path_factory):
    from rocco_amd.readtracks import AlignmentRecords

    arrays, meta = iv.load_golden()
    work = tmp_path_factory.mktemp("score_peaks_from_records")
    paths = {}
    for name, key in (("peaks", "peaks_text"), ("sizes", "sizes_text"), ("summits", "summit_offsets_text")):
        paths[name] = str(work / name)
        with open(paths[name], "w", encoding="utf-8") as handle:
            handle.write(meta[key])
    records = [{contig: AlignmentRecords(*iv.fields_of(arrays, key, contig)) for contig in meta["contigs"]} for key in meta["sample_names"]]
    return arrays, meta, work, paths, records


def test_raw_count_matrix_bytes(scenario):
    from rocco_amd import scores

    arrays, meta, work, paths, records = scenario
    want = arrays["raw_count_matrix_tsv"].tobytes()
    for per_call in (None, 1, 2):
        out = str(work / f"counts_{per_call}.tsv")
        assert scores.raw_count_matrix_from_records(records, meta["sample_names"], paths["peaks"], out, bed_columns=3,
                                                    files_per_call=per_call) == out
        with open(out, "rb") as handle:
            assert handle.read() == want, per_call


def test_get_ecdf_values(scenario):
    from rocco_amd import scores

    arrays, meta, _, paths, records = scenario
    for case in meta["get_ecdf"]:
        for per_call in (None, 1):
            null = scores.get_ecdf_from_records(records, chrom_sizes_file=paths["sizes"], files_per_call=per_call, **case["kwargs"])
            assert isinstance(null, scores.EmpiricalNull) and np.array_equal(null.values, arrays[f"ecdf_{case['name']}_values"]), case
    # a caller's own statistic gets the transformed rows on the host: the default one, passed as another callable
    case = meta["get_ecdf"][0]
    null = scores.get_ecdf_from_records(records, chrom_sizes_file=paths["sizes"], null_stat=lambda row: np.percentile(row, 75.0),
                                        **case["kwargs"])
    assert np.array_equal(null.values, arrays[f"ecdf_{case['name']}_values"])


def test_multi_ecdf_values(scenario):
    from rocco_amd import scores

    arrays, meta, _, paths, records = scenario
    kw = meta["score_peaks"]["kwargs"]
    lengths = arrays["score_peaks_null_lengths"]
    for per_call in (None, 1):
        nulls = scores.multi_ecdf_from_records(records, np.repeat(lengths, 2), paths["sizes"], nsamples_per_length=kw["ecdf_nsamples"],
                                               sample_scaling_constants=arrays["score_peaks_constants"], seed=kw["seed"],
                                               row_scale=kw["row_scale"], pc=kw["pc"], files_per_call=per_call)
        assert [int(k) for k in nulls] == [int(k) for k in lengths]
        for length in lengths:
            assert np.array_equal(nulls[length].values, arrays[f"score_peaks_null_{int(length)}"]), (per_call, int(length))


def test_score_peaks_bytes(scenario):
    from rocco_amd import scores

    arrays, meta, work, paths, records = scenario
    sp = meta["score_peaks"]
    outputs = []
    for per_call in (None, 1):
        out, tsv = str(work / f"scored_{per_call}.bed"), str(work / f"matrix_{per_call}.tsv")
        got = scores.score_peaks_from_records(records, meta["sample_names"], paths["sizes"], paths["peaks"], sp["mapped_counts"],
                                              sp["read_lengths"], count_matrix_file=tsv, output_file=out,
                                              summit_offsets_file=paths["summits"], files_per_call=per_call, **sp["kwargs"])
        with open(out, "rb") as handle:
            outputs.append(handle.read())
        with open(tsv, "rb") as handle:
            assert handle.read() == arrays["raw_count_matrix_tsv"].tobytes()
        for mine, theirs in zip(got, (arrays["score_peaks_scores"], arrays["score_peaks_bed6"], arrays["score_peaks_pvals"])):
            assert np.array_equal(np.asarray(mine), theirs), per_call
    assert outputs[0] == arrays["score_peaks_narrowpeak"].tobytes()
    assert outputs[1] == outputs[0]
    # the matrix written above is read back on the next call (the reference's first branch): the same file again
    out = str(work / "scored_again.bed")
    scores.score_peaks_from_records(records, meta["sample_names"], paths["sizes"], paths["peaks"], sp["mapped_counts"], sp["read_lengths"],
                                    count_matrix_file=str(work / "matrix_None.tsv"), output_file=out,
                                    summit_offsets_file=paths["summits"], **sp["kwargs"])
    with open(out, "rb") as handle:
        assert handle.read() == outputs[0]
