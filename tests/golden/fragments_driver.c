/* tests/golden/fragments_driver.c -- command-line driver that tests/golden/make_golden_fragments.py links against the
 * REFERENCE's compiled counter (its native/ccounts_backend.c) and its vendored htslib.  This file is this project's own: it
 * only calls the reference's public C entry points and htslib's API, and prints / stores what they return.
 *
 *   driver pack IN.txt OUT.tsv.gz [CUT ...]           text -> BGZF (a block ends behind every CUT bytes of the text, given
 *                                                      ascending; htslib's own 0xff00-byte blocks otherwise) + OUT.tsv.gz.tbi
 *                                                      through tbx_index_build with tbx_conf_bed
 *   driver compress IN.txt OUT.tsv.gz                  text -> BGZF, no index (htslib refuses to index a line that ends before it begins)
 *   driver dump PATH CONTIG OUT.txt                   the lines the index iterator yields for the whole CONTIG, '\n' behind each
 *   driver range PATH ALLOW CONTIG CHROM_LEN           prints "start end" of ccounts_getChromRange
 *   driver count PATH ALLOW CONTIG START END STEP LENGTH OUT.f32 MODE ONE_READ_PER_BIN
 *                                                      LENGTH float32 counts of ccounts_countRegion into a zeroed buffer
 *   driver mapped PATH ALLOW MODE ONE_READ_PER_BIN [EXCLUDE ...]   prints "mapped unmapped" of ccounts_getMappedReadCount
 *   driver readlen PATH MIN_READS MAX_ITERATIONS       prints ccounts_getReadLength
 * ALLOW: the barcode allow-list file, "-" for none.  Every call has sourceKind = ccounts_sourceKindFragments.  Where the
 * reference reports an error the driver prints "ERROR <message>" and exits with 0, so that the message can be stored. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <htslib/bgzf.h>
#include <htslib/hts.h>
#include <htslib/kstring.h>
#include <htslib/tbx.h>

#include "ccounts_backend.h"

static int fail(const char *what)
{
    fprintf(stderr, "fragments_driver: %s\n", what);
    return 1;
}

static int refused(ccounts_result result)
{
    printf("ERROR %s\n", result.errorMessage != NULL ? result.errorMessage : "");
    return 0;
}

static ccounts_sourceConfig source_of(const char *path, const char *allow)
{
    ccounts_sourceConfig config;
    memset(&config, 0, sizeof(config));
    config.path = path;
    config.sourceKind = ccounts_sourceKindFragments;
    config.barcodeAllowListFile = strcmp(allow, "-") == 0 ? NULL : allow;
    return config;
}

static int pack(const char *in_path, const char *out_path, int n_cuts, char **cuts, int with_index)
{
    FILE *in = fopen(in_path, "rb");
    if (in == NULL) {
        return fail("cannot open the text");
    }
    fseek(in, 0, SEEK_END);
    const long size = ftell(in);
    fseek(in, 0, SEEK_SET);
    char *text = (char *)malloc((size_t)size + 1);
    if (text == NULL || fread(text, 1, (size_t)size, in) != (size_t)size) {
        return fail("cannot read the text");
    }
    fclose(in);
    BGZF *out = bgzf_open(out_path, "w");
    if (out == NULL) {
        return fail("cannot open the output");
    }
    long at = 0;
    for (int k = 0; k <= n_cuts; ++k) {
        const long upto = k < n_cuts ? atol(cuts[k]) : size;
        if (upto < at || upto > size) {
            return fail("the cuts must ascend within the text");
        }
        if (upto > at && bgzf_write(out, text + at, (size_t)(upto - at)) < 0) {
            return fail("cannot write");
        }
        if (bgzf_flush(out) < 0) {
            return fail("cannot end a block");
        }
        at = upto;
    }
    free(text);
    if (bgzf_close(out) < 0) {
        return fail("cannot finish the output");
    }
    return with_index && tbx_index_build(out_path, 0, &tbx_conf_bed) != 0 ? fail("cannot build the index") : 0;
}

static int dump(const char *path, const char *contig, const char *out_path)
{
    htsFile *in = hts_open(path, "r");
    tbx_t *index = tbx_index_load(path);
    FILE *out = fopen(out_path, "wb");
    if (in == NULL || index == NULL || out == NULL) {
        return fail("cannot open the source, its index or the output");
    }
    hts_itr_t *iterator = tbx_itr_querys(index, contig);
    kstring_t line = {0, 0, NULL};
    while (iterator != NULL && tbx_itr_next(in, index, iterator, &line) >= 0) {
        fwrite(line.s, 1, line.l, out);
        fputc('\n', out);
    }
    if (iterator != NULL) {
        hts_itr_destroy(iterator);
    }
    free(line.s);
    tbx_destroy(index);
    hts_close(in);
    fclose(out);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 4 && strcmp(argv[1], "pack") == 0) {
        return pack(argv[2], argv[3], argc - 4, argv + 4, 1);
    }
    if (argc == 4 && strcmp(argv[1], "compress") == 0) {
        return pack(argv[2], argv[3], 0, NULL, 0);
    }
    if (argc == 5 && strcmp(argv[1], "dump") == 0) {
        return dump(argv[2], argv[3], argv[4]);
    }
    if (argc == 6 && strcmp(argv[1], "range") == 0) {
        ccounts_sourceConfig config = source_of(argv[2], argv[3]);
        uint64_t start = 0, end = 0;
        ccounts_result result = ccounts_getChromRange(&config, argv[4], (uint64_t)strtoull(argv[5], NULL, 10), 1, 0, &start, &end);
        if (result.errorCode != 0) {
            return refused(result);
        }
        printf("%llu %llu\n", (unsigned long long)start, (unsigned long long)end);
        return 0;
    }
    if (argc == 12 && strcmp(argv[1], "count") == 0) {
        ccounts_sourceConfig config = source_of(argv[2], argv[3]);
        ccounts_region region;
        ccounts_countOptions options;
        memset(&options, 0, sizeof(options));
        region.chromosome = argv[4];
        region.start = (uint32_t)strtoul(argv[5], NULL, 10);
        region.end = (uint32_t)strtoul(argv[6], NULL, 10);
        region.intervalSizeBP = (uint32_t)strtoul(argv[7], NULL, 10);
        const size_t length = (size_t)strtoull(argv[8], NULL, 10);
        options.countMode = (uint8_t)atoi(argv[10]);
        options.oneReadPerBin = (uint8_t)(atoi(argv[11]) != 0);
        options.maxInsertSize = 1000;
        options.minTemplateLength = -1;
        float *counts = (float *)calloc(length + 1, sizeof(float));
        ccounts_sourceHandle *handle = NULL;
        ccounts_result result = ccounts_openSource(&config, &handle);
        if (result.errorCode == 0) {
            result = ccounts_countRegion(handle, &region, &options, counts, length);
        }
        if (handle != NULL) {
            ccounts_closeSource(handle);
        }
        if (result.errorCode != 0) {
            return refused(result);
        }
        FILE *out = fopen(argv[9], "wb");
        if (out == NULL || fwrite(counts, sizeof(float), length, out) != length) {
            return fail("cannot write the counts");
        }
        fclose(out);
        free(counts);
        printf("OK\n");
        return 0;
    }
    if (argc >= 6 && strcmp(argv[1], "mapped") == 0) {
        ccounts_sourceConfig config = source_of(argv[2], argv[3]);
        uint64_t mapped = 0, unmapped = 0;
        ccounts_result result = ccounts_getMappedReadCount(&config, 1, (const char *const *)(argv + 6), argc - 6, (uint8_t)atoi(argv[4]),
                                                           (uint8_t)(atoi(argv[5]) != 0), &mapped, &unmapped);
        if (result.errorCode != 0) {
            return refused(result);
        }
        printf("%llu %llu\n", (unsigned long long)mapped, (unsigned long long)unmapped);
        return 0;
    }
    if (argc == 5 && strcmp(argv[1], "readlen") == 0) {
        ccounts_sourceConfig config = source_of(argv[2], "-");
        uint32_t length = 0;
        ccounts_result result = ccounts_getReadLength(&config, 1, atoi(argv[3]), atoi(argv[4]), 0, &length);
        if (result.errorCode != 0) {
            return refused(result);
        }
        printf("%u\n", (unsigned)length);
        return 0;
    }
    return fail("usage: pack | dump | range | count | mapped | readlen (see the head of this file)");
}
