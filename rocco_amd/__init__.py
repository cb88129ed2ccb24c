"""rocco_amd -- MI355X-native implementation of ROCCO's per-chromosome solve path.

Re-exports the hot-path functions under the reference's own names (rocco/__init__.py:1-7 star-exports
them from rocco/dp.py and rocco/rocco.py), so `from rocco_amd import solve_chrom_exact` replaces
`from rocco import solve_chrom_exact`.
"""
from .dp import (  # noqa: F401
    build_switch_costs,
    calibrate_selection_penalty,
    objective_value,
    solve_chrom_exact,
    solve_penalized_chain,
)
from .budget import (  # noqa: F401  (rocco/inference.py:988-1148, 1312-1485, 1593-1737)
    estimate_budget_nonnull_fraction_from_empirical_null,
    estimate_budget_nonnull_fraction_from_resampled_null,
    estimate_budget_nonnull_fraction_from_score_track,
    estimate_budget_nonnull_fraction_from_wild_bootstrap_null,
    estimate_empirical_bayes_budgets,
)
from .inference import crossfit_whittaker_baseline  # noqa: F401  (rocco/_baseline.c:16-104)
from .inference import score_centered_wls  # noqa: F401  (rocco/_wls.c)
from .inference import score_loci_wls  # noqa: F401  (rocco/inference.py:302-379)
from .inference import (  # noqa: F401  (rocco/inference.py:32-37, 382-443, and their tensor-in, tensor-out forms)
    _robust_scale,
    _robust_scale_device,
    _standardize_wls_z_scores,
    _standardize_wls_z_scores_device,
    benjamini_hochberg,
    benjamini_hochberg_device,
    candidate_mask_from_wls,
    candidate_mask_from_wls_device,
)
from .scores import EmpiricalNull, score_peak_counts  # noqa: F401  (rocco/scores.py:120-149, 560-625)
from .readtracks import assemble_chrom_matrix, bigwig_dense_fill  # noqa: F401  (rocco/readtracks.py:141-186, 614-633)
from .readtracks import (  # noqa: F401  (rocco/native/ccounts_backend.c:1666-1705, 2400-2573; rocco/readtracks.py:439-518)
    AlignmentRecords,
    alignment_chrom_range_from_records,
    bam_chrom_reads_from_records,
    bam_chrom_reads_from_records_batch,
    count_alignment_records_batch_device,
    count_alignment_region_from_records,
)
from .readtracks import (  # noqa: F401  (rocco/native/ccounts_backend.c:598-1524, 1712-1888; rocco/readtracks.py:242-353)
    AlignmentFileRecords,
    alignment_fragment_length_from_records,
    alignment_fragment_length_from_records_batch,
    alignment_mapped_read_count_from_records,
    alignment_read_length_from_records,
    bam_count_metadata_from_records,
    bam_count_metadata_from_records_batch,
    is_alignment_paired_end_from_records,
)
from .bam import (  # noqa: F401  (htslib's BGZF reader, bam_read1, bam_endpos, bam_cigar2qlen; rocco/readtracks.py:242-518)
    clear_alignment_cache,
    get_bam_chrom_reads,
    inflate_bgzf,
    inflate_bgzf_device,
    parse_bam_header,
    read_alignment_file,
    read_alignment_spans,
    IndexedAlignmentFile,
)
from .bam_index import (  # noqa: F401  (htslib's BAI reader: hts_idx_load, hts_idx_get_stat, the pseudo-bin's offsets)
    clear_bam_index_cache,
    contig_span,
    contig_stats,
    open_bam_index,
)
from .bigwig import (  # noqa: F401  (what libBigWig does behind pyBigWig's intervals(): the data blocks, their intervals)
    clear_bigwig_cache,
    open_bigwig,
    read_bigwig_blocks,
    read_bigwig_intervals,
    read_bigwig_intervals_batch,
)
from .rocco import (  # noqa: F401
    chrom_solution_to_bed,
    combine_chrom_results,
    cscores_quantiles,
    cscores_quantiles_batch_device,
    generate_narrowpeak_if_requested,
    run_to_narrowpeak,
    score_central_tendency_chrom,
    score_dispersion_chrom,
    solve_cached_chromosomes,
)

__version__ = "0.1.0"
