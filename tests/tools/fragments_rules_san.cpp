// tests/tools/fragments_rules_san.cpp -- rocco_amd/csrc/fragments_rules.h, the rules the kernels of fragments_file.hip compile,
// in one stand-alone executable for the host's sanitizers (tests/test_fragments_host.py builds it with
// -fsanitize=address,undefined and runs it over `.case` files).  CPU only; nothing of HIP is needed.
//
// A `.case` file (little-endian, written by tests/test_fragments_host.py): 13 int64 -- n_bytes, entry0, whole_file, n_names,
// name_bytes, n_allow, allow_bytes, expect, n_lines, cut, open, report line, report code --, then the text, the n_names + 1
// name offsets (int64) and the names' bytes, the n_allow + 1 allow-list offsets (int64) and its bytes, and what is expected:
// n_lines + 1 starts (int64), then start, end, weight, name (int32 each) and status (uint32) per line.  Every input and output
// is allocated at exactly its size, so that a read or write one element past any of them is an error the sanitizer names.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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
    int64_t head[13];
    if (fread(head, sizeof(int64_t), 13, in) != 13) {
        fprintf(stderr, "%s: no header\n", path);
        return 1;
    }
    const size_t n_bytes = (size_t)head[0], entry0 = (size_t)head[1], n_names = (size_t)head[3], name_bytes = (size_t)head[4],
                 n_allow = (size_t)head[5], allow_bytes_n = (size_t)head[6], n_lines = (size_t)head[8];
    const int whole_file = (int)head[2];
    const int32_t expect = (int32_t)head[7];
    uint8_t *bytes = exact<uint8_t>(n_bytes), *names = exact<uint8_t>(name_bytes), *allow_bytes = exact<uint8_t>(allow_bytes_n);
    int64_t *name_offsets = exact<int64_t>(n_names + 1), *allow_offsets = exact<int64_t>(n_allow + 1), *want_starts = exact<int64_t>(n_lines + 1);
    int32_t *want[4];
    for (int q = 0; q < 4; ++q) {
        want[q] = exact<int32_t>(n_lines);
    }
    uint32_t *want_status = exact<uint32_t>(n_lines);
    bool ok = read_array(in, bytes, n_bytes) && read_array(in, name_offsets, n_names + 1) && read_array(in, names, name_bytes) &&
              read_array(in, allow_offsets, n_allow + 1) && read_array(in, allow_bytes, allow_bytes_n) && read_array(in, want_starts, n_lines + 1);
    for (int q = 0; q < 4; ++q) {
        ok = ok && read_array(in, want[q], n_lines);
    }
    ok = ok && read_array(in, want_status, n_lines);
    fclose(in);
    if (!ok) {
        fprintf(stderr, "%s: cut short\n", path);
        return 1;
    }
    int bad = 0;
    int64_t lines_report[4], fields_report[4];
    rocco::fragfile_lines_host(bytes, n_bytes, entry0, nullptr, 0, lines_report);
    if (lines_report[0] != head[8] || lines_report[1] != head[9] || lines_report[2] != head[10]) {
        fprintf(stderr, "%s: the line report is %lld %lld %lld\n", path, (long long)lines_report[0], (long long)lines_report[1], (long long)lines_report[2]);
        ++bad;
    }
    int64_t *starts = exact<int64_t>(n_lines + 1);
    if (!rocco::fragfile_lines_host(bytes, n_bytes, entry0, starts, n_lines + 1, lines_report) ||
        memcmp(starts, want_starts, (n_lines + 1) * sizeof(int64_t)) != 0) {
        fprintf(stderr, "%s: the line starts differ\n", path);
        ++bad;
    }
    if (n_lines > 0 && rocco::fragfile_lines_host(bytes, n_bytes, entry0, starts, n_lines, lines_report)) {
        fprintf(stderr, "%s: a capacity one short was accepted\n", path);
        ++bad;
    }
    int32_t *got[4];
    for (int q = 0; q < 4; ++q) {
        got[q] = exact<int32_t>(n_lines);
    }
    uint32_t *status = exact<uint32_t>(n_lines);
    const int64_t track_first[2] = {0, (int64_t)n_lines}, allow_first[2] = {0, (int64_t)n_allow};
    const rocco::FragNames table = {names, name_offsets, 0, (long long)n_names};
    if (bad == 0) {
        rocco::fragfile_fields_host(bytes, starts, n_lines, whole_file, track_first, &expect, 1, table, allow_bytes, allow_offsets, allow_first, got[0],
                                    got[1], got[2], got[3], status, fields_report);
        if (fields_report[0] != head[11] || fields_report[1] != head[12]) {
            fprintf(stderr, "%s: the field report is %lld %lld\n", path, (long long)fields_report[0], (long long)fields_report[1]);
            ++bad;
        }
        for (int q = 0; q < 4; ++q) {
            if (n_lines > 0 && memcmp(got[q], want[q], n_lines * sizeof(int32_t)) != 0) {
                fprintf(stderr, "%s: field array %d differs\n", path, q);
                ++bad;
            }
        }
        if (n_lines > 0 && memcmp(status, want_status, n_lines * sizeof(uint32_t)) != 0) {
            fprintf(stderr, "%s: the status words differ\n", path);
            ++bad;
        }
        // the bin arithmetic of every mode over what was parsed, at regions that cut, clamp and miss (its results are the
        // GPU tests' to compare; here it runs under the sanitizers)
        long long sink = 0;
        for (size_t i = 0; i < n_lines; ++i) {
            if (!rocco::frag_valid_count(status[i], got[0][i], got[1][i])) {
                continue;
            }
            for (int mode = 0; mode < 4; ++mode) {
                for (int one = 0; one < 2; ++one) {
                    const rocco::FragCells a = rocco::frag_cells(got[0][i], got[1][i], mode, one, 1237, 61761, 10, 6053);
                    const rocco::FragCells b = rocco::frag_cells(got[0][i], got[1][i], mode, one, 0, 2147483646, 1, 17);
                    sink += a.n_plus + b.n_plus + a.minus + b.minus + rocco::frag_mapped_weight(got[2][i], mode, one);
                }
            }
            sink += rocco::frag_valid_mapped(status[i], got[3][i]) + rocco::frag_valid_read_length(status[i], got[0][i], got[1][i]);
        }
        if (sink == 0x7fffffffffffffffLL) {
            printf(" ");
        }
    }
    free(bytes);
    free(names);
    free(allow_bytes);
    free(name_offsets);
    free(allow_offsets);
    free(want_starts);
    free(want_status);
    free(starts);
    free(status);
    for (int q = 0; q < 4; ++q) {
        free(want[q]);
        free(got[q]);
    }
    return bad;
}

}  // namespace

int main(int argc, char **argv)
{
    int bad = 0;
    for (int k = 1; k < argc; ++k) {
        bad += run_case(argv[k]);
    }
    printf("%d files, %s\n", argc - 1, bad == 0 ? "all as expected" : "DIFFERENCES");
    return bad == 0 ? 0 : 1;
}
