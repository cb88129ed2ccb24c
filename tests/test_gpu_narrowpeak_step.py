"""Row f12 on the GPU: the driver's last step.  `rocco_amd.rocco.generate_narrowpeak_if_requested` against the files and
log records the reference's `_generate_narrowpeak_if_requested` left for the same BAM files, BED and summit tracks
(tests/golden/score_paths.*), and `run_to_narrowpeak` from BAM paths against `run_chromosomes` and `score_peaks` called by
hand.  File bytes and log records are compared exactly."""
import glob
import os
import tempfile

import pytest

import score_paths_files as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def paths(gpu, tmp_path_factory):
    from rocco_amd import bam

    bam.clear_alignment_cache()
    yield sp.write_files(tmp_path_factory.mktemp("narrowpeak_step"))
    bam.clear_alignment_cache()


def temp_files():
    return sorted(glob.glob(os.path.join(tempfile.gettempdir(), "rocco_pointsource_*")) +
                  glob.glob(os.path.join(tempfile.gettempdir(), "rocco_summit_track_*")))


def file_bytes(path):
    with open(path, "rb") as handle:
        return handle.read()


@pytest.mark.parametrize("case", [0, 1, 2, 3, 4])
def test_step_against_the_references_files_and_log(paths, case):
    from rocco_amd import rocco as impl

    arrays, meta = sp.golden()
    entry = meta["narrowpeak"][case]
    folder = os.path.join(paths["dir"], "np_" + entry["name"])
    os.mkdir(folder)
    final_output = os.path.join(folder, entry["output"])
    with open(final_output, "w") as handle:
        handle.write(meta["narrowpeak_bed_text"])
    before = temp_files()
    cache = {contig: {"summit_track_file": impl._cpy_narrowpeak_summit_track(contig, arrays[f"np_track_{contig}_intervals"],
                                                                            arrays[f"np_track_{contig}_mean"])} for contig in ("chr1", "chr2")}
    inputs = [paths[k] for k in sp.FILES] + ([os.path.join(paths["dir"], "missing.bam")] if entry["missing_input"] else [])
    args = {"narrowPeak": True, "input_track_type": entry["input_track_type"], "input_files": inputs, "chrom_sizes_file": paths["g.sizes"],
            "ecdf_samples": 25, "ecdf_seed": 13, "ecdf_proc": 1}
    try:
        written, log = sp.logged(lambda: impl.generate_narrowpeak_if_requested(args, final_output, cache), paths["dir"])
    finally:
        for chrom_data in cache.values():
            os.remove(chrom_data["summit_track_file"])
    assert log == entry["log"]
    assert sorted(f for f in os.listdir(folder) if f != entry["output"]) == entry["files"]
    for produced in entry["files"]:
        assert file_bytes(os.path.join(folder, produced)) == arrays[f"np_{entry['name']}_{produced}"].tobytes(), produced
    if entry["files"]:
        assert written == os.path.join(folder, [f for f in entry["files"] if f.endswith(".narrowPeak")][0])
    else:
        assert written is None
    assert temp_files() == before  # the offsets file is removed, also behind a failure
    assert impl.generate_narrowpeak_if_requested(dict(args, narrowPeak=False), final_output, cache) is None
    assert sorted(f for f in os.listdir(folder) if f != entry["output"]) == entry["files"]


def test_run_to_narrowpeak_from_bam_paths(paths, tmp_path, monkeypatch):
    """The BED of `run_chromosomes`, byte for byte; the narrowPeak `score_peaks` writes by hand for that BED with the same
    summit offsets; no summit track and no offsets file left behind."""
    from rocco_amd import bam
    from rocco_amd import rocco as impl
    from rocco_amd import scores

    chroms = ["chr1", "chr2"]
    inputs = [paths[k] for k in sp.FILES]
    args = {"chrom_sizes_file": paths["g.sizes"], "step": 50, "round_digits": 5, "effective_genome_size": -1, "norm_method": "CPM",
            "min_mapping_score": 10, "flag_include": None, "flag_exclude": 3844, "extend_reads": -1, "center_reads": False,
            "ignore_for_norm": None, "scale_factor": 1.0, "score_lower_bound_z": 1.0, "score_prior_df": 6.0, "score_min_effect": None,
            "score_precision_floor_ratio": 0.01, "gamma": None, "budget": None, "scale_chrom_budgets": 1.0,
            "budget_posterior_quantile": 0.01, "selection_penalty": None, "min_length_bp": 100, "narrowPeak": True, "low_memory": False,
            "input_track_type": "bam", "budget_null_draws": 6, "threads": 1, "input_files": inputs, "ecdf_samples": 20, "ecdf_seed": 4,
            "ecdf_proc": 1}
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(impl, "generate_chrom_matrix", bam.generate_chrom_matrix_device)
    before = temp_files()
    want_bed = impl.run_chromosomes(chroms, inputs, dict(args, output=str(tmp_path / "want.bed")), run_id="1")
    # the summit offsets the step hands to score_peaks: kept from its own call
    kept = {}
    write = impl._write_narrowpeak_summit_offsets

    def keeping(peak_file, chrom_cache, output_file):
        out = write(peak_file, chrom_cache, output_file)
        kept["offsets"] = file_bytes(output_file)
        return out

    monkeypatch.setattr(impl, "_write_narrowpeak_summit_offsets", keeping)
    got_bed, narrowpeak = impl.run_to_narrowpeak(chroms, inputs, dict(args, output=str(tmp_path / "got.bed")), run_id="2")
    assert got_bed == str(tmp_path / "got.bed") and narrowpeak == str(tmp_path / "got.narrowPeak")
    assert len(file_bytes(want_bed)) > 0 and file_bytes(got_bed) == file_bytes(want_bed)
    assert temp_files() == before
    assert sorted(os.listdir(tmp_path)) == ["got.bed", "got.counts.tsv", "got.narrowPeak", "want.bed"]
    offsets = tmp_path / "offsets.tsv"
    offsets.write_bytes(kept["offsets"])
    assert len(kept["offsets"].splitlines()) == len(file_bytes(got_bed).splitlines())
    scores.score_peaks(inputs, paths["g.sizes"], want_bed, count_matrix_file=str(tmp_path / "hand.counts.tsv"),
                       output_file=str(tmp_path / "hand.narrowPeak"), ecdf_nsamples=20, seed=4, proc=1, summit_offsets_file=str(offsets))
    assert file_bytes(narrowpeak) == file_bytes(tmp_path / "hand.narrowPeak")
    assert file_bytes(tmp_path / "got.counts.tsv") == file_bytes(tmp_path / "hand.counts.tsv")
    # narrowPeak not asked for: the BED alone, and None
    got_bed, narrowpeak = impl.run_to_narrowpeak(chroms, inputs, dict(args, narrowPeak=False, output=str(tmp_path / "plain.bed")), run_id="3")
    assert narrowpeak is None and file_bytes(got_bed) == file_bytes(want_bed) and not os.path.exists(tmp_path / "plain.narrowPeak")
    assert temp_files() == before


def test_run_to_narrowpeak_is_single_process(gpu, monkeypatch):
    from rocco_amd import rocco as impl

    monkeypatch.setattr(impl, "_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="single-process"):
        impl.run_to_narrowpeak(["chr1"], {}, {"narrowPeak": True, "output": "never.bed"})
