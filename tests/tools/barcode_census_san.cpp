// tests/tools/barcode_census_san.cpp -- the census part of rocco_amd/csrc/fragments_rules.h (frag_barcode_field, frag_hash64,
// barcode_census_host: what the kernels of barcode_census.hip compile, and their host twin) in one stand-alone executable for
// the host's sanitizers (tests/test_barcode_census_host.py builds it with -fsanitize=address,undefined and runs it over
// `.case` files).  CPU only; nothing of HIP is needed.
//
// A `.case` file (little-endian, written by tests/test_barcode_census_host.py): 8 int64 -- n_bytes, n_allow, allow_bytes,
// hash_mask (its bit pattern), initial_capacity, entries, barcode bytes, lines --, then the text, the n_allow + 1 allow-list
// offsets (int64) and its bytes, and what is expected in the order of first lines: the barcodes' bytes, entries + 1 offsets
// (int64), entries records (int64).  Every input and output is allocated at exactly its size, so that a read or write one
// element past any of them is an error the sanitizer names.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../rocco_amd/csrc/fragments_rules.h"

namespace {

template <class T>
T *exact(size_t n)
{
    return n == 0 ? nullptr : (T *)malloc(n * sizeof(T));
}

template <class T>
bool read_array(FILE *in, T *to, size_t n)
{
    return n == 0 || fread(to, sizeof(T), n, in) == n;
}

int run_case(const char *path)
{
    FILE *in = fopen(path, "rb");
    if (in == nullptr) {
        fprintf(stderr, "%s: cannot open\n", path);
        return 1;
    }
    int64_t head[8];
    if (fread(head, sizeof(int64_t), 8, in) != 8) {
        fprintf(stderr, "%s: no header\n", path);
        return 1;
    }
    const size_t n_bytes = (size_t)head[0], n_allow = (size_t)head[1], allow_bytes_n = (size_t)head[2], entries = (size_t)head[5],
                 total = (size_t)head[6];
    const uint64_t hash_mask = (uint64_t)head[3], initial_capacity = (uint64_t)head[4];
    uint8_t *bytes = exact<uint8_t>(n_bytes), *allow_bytes = exact<uint8_t>(allow_bytes_n), *want_bytes = exact<uint8_t>(total);
    int64_t *allow_offsets = exact<int64_t>(n_allow + 1), *want_offsets = exact<int64_t>(entries + 1), *want_records = exact<int64_t>(entries);
    const bool ok = read_array(in, bytes, n_bytes) && read_array(in, allow_offsets, n_allow + 1) && read_array(in, allow_bytes, allow_bytes_n) &&
                    read_array(in, want_bytes, total) && read_array(in, want_offsets, entries + 1) && read_array(in, want_records, entries);
    fclose(in);
    if (!ok) {
        fprintf(stderr, "%s: cut short\n", path);
        return 1;
    }
    const rocco::FragNames allow = {allow_bytes, allow_offsets, 0, (long long)n_allow};
    int failed = 0;
    int64_t report[4] = {-1, -1, -1, -1};
    if (!rocco::barcode_census_host(bytes, n_bytes, allow, hash_mask, initial_capacity, nullptr, 0, nullptr, nullptr, 0, report) ||
        report[0] != head[5] || report[1] != head[6] || report[2] != head[7]) {
        fprintf(stderr, "%s: the sizes: %lld entries, %lld bytes, %lld lines\n", path, (long long)report[0], (long long)report[1], (long long)report[2]);
        failed = 1;
    }
    uint8_t *got_bytes = exact<uint8_t>(total);
    int64_t *got_offsets = exact<int64_t>(entries + 1), *got_records = exact<int64_t>(entries);
    if (!failed && (!rocco::barcode_census_host(bytes, n_bytes, allow, hash_mask, initial_capacity, got_bytes, total, got_offsets, got_records,
                                                entries, report) ||
                    (total > 0 && memcmp(got_bytes, want_bytes, total) != 0) || memcmp(got_offsets, want_offsets, (entries + 1) * sizeof(int64_t)) != 0 ||
                    (entries > 0 && memcmp(got_records, want_records, entries * sizeof(int64_t)) != 0))) {
        fprintf(stderr, "%s: the arrays differ\n", path);
        failed = 1;
    }
    // an output one entry (one byte) short is refused and nothing is written
    if (!failed && entries > 0 &&
        (rocco::barcode_census_host(bytes, n_bytes, allow, hash_mask, initial_capacity, got_bytes, total, got_offsets, got_records, entries - 1, report) ||
         rocco::barcode_census_host(bytes, n_bytes, allow, hash_mask, initial_capacity, got_bytes, total - 1, got_offsets, got_records, entries, report))) {
        fprintf(stderr, "%s: an output too small was accepted\n", path);
        failed = 1;
    }
    // the field rule and the hash on every line of the text, and on every line without its last byte
    size_t p = 0;
    uint64_t mixed = 0;
    while (p < n_bytes) {
        size_t end = p;
        while (end < n_bytes && bytes[end] != '\n') {
            ++end;
        }
        const long long length = (long long)(end < n_bytes ? end + 1 : end) - (long long)p;
        for (long long cut = 0; cut < 2 && cut <= length; ++cut) {
            long long offset = 0, n = 0;
            if (rocco::frag_barcode_field(bytes + p, length - cut, &offset, &n)) {
                if (offset < 0 || n <= 0 || offset + n > length - cut) {
                    fprintf(stderr, "%s: a barcode outside its line\n", path);
                    failed = 1;
                }
                mixed ^= rocco::frag_hash64(bytes + p + offset, n);
            }
        }
        p = end < n_bytes ? end + 1 : end;
    }
    if (mixed == 1) {
        printf(" ");  // (the hashes are used)
    }
    free(bytes);
    free(allow_bytes);
    free(want_bytes);
    free(allow_offsets);
    free(want_offsets);
    free(want_records);
    free(got_bytes);
    free(got_offsets);
    free(got_records);
    return failed;
}

}  // namespace

int main(int argc, char **argv)
{
    int failed = 0;
    for (int k = 1; k < argc; ++k) {
        failed += run_case(argv[k]);
    }
    printf("%d files, %s\n", argc - 1, failed == 0 ? "all as expected" : "FAILED");
    return failed == 0 ? 0 : 1;
}
