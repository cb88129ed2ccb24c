// rocco_amd/csrc/count_tail.h -- the scaling of get_bam_chrom_reads' tail (rocco/readtracks.py:492-503) for one bin, stated
// once: count_tail_kernel and track_supports_kernel (count.hip) and track_matrix_fill_kernel (track_matrix.hip) call it.
#pragma once

#include <hip/hip_runtime.h>

namespace rocco {

// vals = counts.astype(float64) * norm_scale; / float(step) when scale_by_step; * const_scale when const_scale >= 0
// (apply_const), in that order.  A bin belongs to the support iff the result is > 0 (before rounding): a zero or negative
// scale or an underflow gives none, whatever the count.
__device__ __forceinline__ double count_tail_value(float count, double norm_scale, int scale_by_step, double step, int apply_const,
                                                   double const_scale)
{
    double v = (double)count;
    v = v * norm_scale;
    if (scale_by_step) {
        v = v / step;
    }
    if (apply_const) {
        v = v * const_scale;
    }
    return v;
}

}  // namespace rocco
