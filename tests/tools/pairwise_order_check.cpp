// tests/tools/pairwise_order_check.cpp -- rocco_amd/csrc/pairwise_sum.h, the summation order the kernels of dispersion.hip
// compile, run on the host for every length the entry points take.
//
//   pairwise_order_check FILE      FILE: float64 values, native byte order, at least kPairwiseMax of them
//
// prints kPairwiseMax lines "n bits": the sum of the first n values at the depth the kernels use, as the 16 hex digits of its
// bit pattern.  tests/test_dispersion_host.py compares every line with np.sum of the same prefix.  Build with
// -ffp-contract=off (the kernels' own setting): every addition rounds where it is written.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rocco_amd/csrc/pairwise_sum.h"

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s FILE\n", argv[0]);
        return 2;
    }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    std::vector<double> values(rocco::kPairwiseMax);
    const size_t got = std::fread(values.data(), sizeof(double), values.size(), f);
    std::fclose(f);
    if (got != values.size()) {
        std::fprintf(stderr, "%s holds %zu values, %d wanted\n", argv[1], got, rocco::kPairwiseMax);
        return 2;
    }
    const double *v = values.data();
    for (int n = 1; n <= rocco::kPairwiseMax; ++n) {
        const double sum = rocco::pairwise<rocco::kPairwiseDepth>(0, n, [v](int i) -> double { return v[i]; });
        uint64_t bits;
        std::memcpy(&bits, &sum, sizeof bits);
        std::printf("%d %016" PRIx64 "\n", n, bits);
    }
    return 0;
}
