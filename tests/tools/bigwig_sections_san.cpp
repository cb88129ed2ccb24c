// tests/tools/bigwig_sections_san.cpp -- the section decode rules of rocco_amd/csrc/bigwig_sections.h (the source the kernels of
// bigwig_sections.hip compile) under the host's sanitizers, as a stand-alone program (it needs no GPU, nothing is preloaded):
//
//     python tests/bigwig_sections_cases.py DIR
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/tools/bigwig_sections_san.cpp -o bigwig_sections_san
//     ./bigwig_sections_san DIR/*.case
//
// A case file: int64 n_slots, n_blocks, n_files, n_intervals; the slots' bytes; the block table (int64 [n_blocks][5]); produced
// (int64 [n_blocks]); file_first (int64 [n_files + 1]), chrom_id and chrom_length (int64 [n_files]); the expected status per
// block (int32); the expected starts, ends (int64) and values (the float64s' bits, uint64) where no block is refused.  Every
// buffer, the slots and the three outputs among them, is allocated at its exact size: one byte read behind the slots or one
// element written behind an output is an AddressSanitizer report.  A status, an offset or an interval that differs fails too.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../rocco_amd/csrc/bigwig_sections.h"

static bool read_exact(FILE *f, void *to, size_t n) { return n == 0 || fread(to, 1, n, f) == n; }

template <class T>
static T *exact(size_t n)
{
    return (T *)malloc(n * sizeof(T) > 0 ? n * sizeof(T) : 1);
}

int main(int argc, char **argv)
{
    long long blocks = 0, refused = 0, intervals = 0;
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        int64_t head[4];
        if (f == nullptr || !read_exact(f, head, sizeof(head)) || head[0] < 0 || head[1] < 0 || head[2] < 0 || head[3] < 0) {
            fprintf(stderr, "%s: cannot read\n", argv[a]);
            return 2;
        }
        const size_t n_slots = (size_t)head[0], n = (size_t)head[1], K = (size_t)head[2], m = (size_t)head[3];
        uint8_t *slots = exact<uint8_t>(n_slots);
        int64_t *table = exact<int64_t>(n * ROCCO_ZLIB_TABLE_COLUMNS), *produced = exact<int64_t>(n), *file_first = exact<int64_t>(K + 1);
        int64_t *chrom_id = exact<int64_t>(K), *chrom_length = exact<int64_t>(K), *want_starts = exact<int64_t>(m), *want_ends = exact<int64_t>(m);
        int32_t *want_status = exact<int32_t>(n), *status = exact<int32_t>(n);
        uint64_t *want_values = exact<uint64_t>(m);
        if (!read_exact(f, slots, n_slots) || !read_exact(f, table, n * ROCCO_ZLIB_TABLE_COLUMNS * 8) || !read_exact(f, produced, n * 8) ||
            !read_exact(f, file_first, (K + 1) * 8) || !read_exact(f, chrom_id, K * 8) || !read_exact(f, chrom_length, K * 8) ||
            !read_exact(f, want_status, n * 4) || !read_exact(f, want_starts, m * 8) || !read_exact(f, want_ends, m * 8) ||
            !read_exact(f, want_values, m * 8)) {
            fprintf(stderr, "%s: cut short\n", argv[a]);
            return 2;
        }
        fclose(f);
        if (!rocco::section_files_ok(file_first, K, n)) {
            fprintf(stderr, "%s: the file offsets do not ascend from 0 to the number of blocks\n", argv[a]);
            return 2;
        }
        int64_t *block_first = exact<int64_t>(n + 1), *file_offsets = exact<int64_t>(K + 1), report[ROCCO_BGZF_REPORT];
        // stage 1 alone, then both stages into outputs of exactly the total
        rocco::sections_host(slots, n_slots, table, produced, n, file_first, chrom_id, chrom_length, K, status, block_first, file_offsets, nullptr,
                             nullptr, nullptr, 0, report);
        const size_t total = (size_t)report[2];
        int64_t *starts = exact<int64_t>(total), *ends = exact<int64_t>(total);
        uint64_t *values = exact<uint64_t>(total);
        if (!rocco::sections_host(slots, n_slots, table, produced, n, file_first, chrom_id, chrom_length, K, status, block_first, file_offsets,
                                  starts, ends, values, total, report)) {
            fprintf(stderr, "%s: the second stage refused its own total\n", argv[a]);
            return 1;
        }
        long long first_refused = -1;
        for (size_t k = 0; k < n; ++k) {
            if (status[k] != want_status[k]) {
                fprintf(stderr, "%s: block %zu: status %d, expected %d\n", argv[a], k, status[k], want_status[k]);
                return 1;
            }
            if (status[k] != 0 && first_refused < 0) {
                first_refused = (long long)k;
            }
            refused += status[k] != 0;
        }
        if (report[0] != first_refused || (first_refused >= 0 && report[1] != status[first_refused])) {
            fprintf(stderr, "%s: the report names block %lld, expected %lld\n", argv[a], (long long)report[0], first_refused);
            return 1;
        }
        if (first_refused < 0) {
            if (total != m || file_offsets[K] != (int64_t)m || memcmp(starts, want_starts, m * 8) != 0 || memcmp(ends, want_ends, m * 8) != 0 ||
                memcmp(values, want_values, m * 8) != 0) {
                fprintf(stderr, "%s: %zu intervals, expected %zu, or their values differ\n", argv[a], total, m);
                return 1;
            }
            intervals += (long long)m;
        }
        blocks += (long long)n;
        for (void *p : {(void *)slots, (void *)table, (void *)produced, (void *)file_first, (void *)chrom_id, (void *)chrom_length,
                        (void *)want_starts, (void *)want_ends, (void *)want_status, (void *)status, (void *)want_values, (void *)block_first,
                        (void *)file_offsets, (void *)starts, (void *)ends, (void *)values}) {
            free(p);
        }
    }
    printf("%d files, %lld blocks, %lld refused, %lld intervals, all as expected\n", argc - 1, blocks, refused, intervals);
    return 0;
}
