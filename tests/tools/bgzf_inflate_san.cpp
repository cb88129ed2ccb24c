// tests/tools/bgzf_inflate_san.cpp -- the decode rules of rocco_amd/csrc/inflate_core.h, under both framings, under the host's
// sanitizers, as a stand-alone program (it needs no GPU):
//
//     python tests/tools/bgzf_inflate_cases.py DIR
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/tools/bgzf_inflate_san.cpp -o bgzf_inflate_san
//     ./bgzf_inflate_san DIR/*.case
//
// A case file: int64 framing (0: BGZF rows, 1: zlib rows), n_comp, n_blocks, n_out; the compressed bytes; the block table
// (int64 [n_blocks][5], rocco_hip.h); the expected status code per block (uint8).  Every buffer is allocated at its exact size,
// so a load outside a span's buffer or a store outside the output buffer is an AddressSanitizer report; a status that differs
// from the expected one fails too.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rocco_amd/csrc/inflate_core.h"

static bool read_exact(FILE *f, void *to, size_t n) { return n == 0 || fread(to, 1, n, f) == n; }

int main(int argc, char **argv)
{
    long long blocks = 0, refused = 0;
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        int64_t head[4];
        if (f == nullptr || !read_exact(f, head, sizeof(head)) || head[0] < 0 || head[0] > 1 || head[1] < 0 || head[2] < 0 || head[3] < 0) {
            fprintf(stderr, "%s: cannot read\n", argv[a]);
            return 2;
        }
        static_assert(ROCCO_BGZF_TABLE_COLUMNS == ROCCO_ZLIB_TABLE_COLUMNS, "one table shape for both framings");
        uint8_t *comp = (uint8_t *)malloc((size_t)head[1]), *out = (uint8_t *)malloc((size_t)head[3]);
        std::vector<int64_t> table((size_t)head[2] * ROCCO_BGZF_TABLE_COLUMNS);
        std::vector<uint8_t> want((size_t)head[2]);
        std::vector<int32_t> status((size_t)head[2]);
        if (!read_exact(f, comp, (size_t)head[1]) || !read_exact(f, table.data(), table.size() * sizeof(int64_t)) ||
            !read_exact(f, want.data(), want.size())) {
            fprintf(stderr, "%s: cut short\n", argv[a]);
            return 2;
        }
        fclose(f);
        int64_t report[ROCCO_BGZF_REPORT] = {0};
        (head[0] == 0 ? rocco::inflate_host<rocco::BgzfFraming> : rocco::inflate_host<rocco::ZlibFraming>)(
            comp, head[1], table.data(), head[2], out, head[3], status.data(), nullptr, report);
        for (size_t k = 0; k < status.size(); ++k) {
            if ((status[k] & 0xff) != want[k]) {
                fprintf(stderr, "%s: block %zu: status %d, expected %d\n", argv[a], k, status[k], (int)want[k]);
                return 1;
            }
            refused += status[k] != 0;
        }
        blocks += head[2];
        free(comp);
        free(out);
    }
    printf("%d files, %lld blocks, %lld refused as expected: clean\n", argc - 1, blocks, refused);
    return 0;
}
