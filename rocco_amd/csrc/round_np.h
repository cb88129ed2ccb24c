// rocco_amd/csrc/round_np.h -- np.round(v, digits) for one float64, shared by assemble.hip and count.hip.
#pragma once

#include <hip/hip_runtime.h>

namespace rocco {

// np.round multiplies by 10**d, rounds half to even (np.rint) and divides by 10**d (d > 0), or divides, rounds and
// multiplies (d < 0); pow10 is 10**|d| as NumPy's integer power converted to float64 (exact up to 10**22)
__device__ __forceinline__ double round_like_numpy(double v, double pow10, int digits)
{
    if (digits > 0) {
        return rint(v * pow10) / pow10;
    }
    if (digits == 0) {
        return rint(v);
    }
    return rint(v / pow10) * pow10;
}

inline double numpy_pow10(int digits)
{
    double pow10 = 1.0;
    for (int d = 0; d < (digits < 0 ? -digits : digits); ++d) {
        pow10 *= 10.0;
    }
    return pow10;
}

}  // namespace rocco
