/* tests/golden/barcode_census_driver.c -- command-line driver that tests/golden/make_golden_barcode_census.py links against the
 * REFERENCE's compiled counter (its native/ccounts_backend.c) and its vendored htslib.  This file is this project's own: it
 * only calls the reference's public C entry points and htslib's API, and prints what they return.
 *
 *   driver pack IN.txt OUT.tsv.gz [CUT ...]     text -> BGZF (a block ends behind every CUT bytes of the text, given ascending;
 *                                               htslib's own blocks otherwise) + OUT.tsv.gz.tbi (tbx_index_build, tbx_conf_bed)
 *   driver compress IN.txt OUT.tsv.gz           text -> BGZF, no index
 *   driver cells PATH ALLOW KIND                prints ccounts_getCellCount; KIND: "fragments" or "bam" (the source kind asked for)
 *   driver mapped PATH ALLOW                    prints "mapped unmapped" of ccounts_getMappedReadCount (coverage, nothing excluded)
 * ALLOW: the barcode allow-list file, "-" for none.  Where the reference reports an error the driver prints "ERROR <message>"
 * and exits with 0, so that the message can be stored. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <htslib/bgzf.h>
#include <htslib/hts.h>
#include <htslib/tbx.h>

#include "ccounts_backend.h"

static int fail(const char *what)
{
    fprintf(stderr, "barcode_census_driver: %s\n", what);
    return 1;
}

static int refused(ccounts_result result)
{
    printf("ERROR %s\n", result.errorMessage != NULL ? result.errorMessage : "");
    return 0;
}

static ccounts_sourceConfig source_of(const char *path, const char *allow, const char *kind)
{
    ccounts_sourceConfig config;
    memset(&config, 0, sizeof(config));
    config.path = path;
    config.sourceKind = strcmp(kind, "bam") == 0 ? ccounts_sourceKindBAM : ccounts_sourceKindFragments;
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

int main(int argc, char **argv)
{
    if (argc >= 4 && strcmp(argv[1], "pack") == 0) {
        return pack(argv[2], argv[3], argc - 4, argv + 4, 1);
    }
    if (argc == 4 && strcmp(argv[1], "compress") == 0) {
        return pack(argv[2], argv[3], 0, NULL, 0);
    }
    if (argc == 5 && strcmp(argv[1], "cells") == 0) {
        ccounts_sourceConfig config = source_of(argv[2], argv[3], argv[4]);
        uint64_t cells = 0;
        ccounts_result result = ccounts_getCellCount(&config, &cells);
        if (result.errorCode != 0) {
            return refused(result);
        }
        printf("%llu\n", (unsigned long long)cells);
        return 0;
    }
    if (argc == 4 && strcmp(argv[1], "mapped") == 0) {
        ccounts_sourceConfig config = source_of(argv[2], argv[3], "fragments");
        uint64_t mapped = 0, unmapped = 0;
        ccounts_result result = ccounts_getMappedReadCount(&config, 1, NULL, 0, 0, 0, &mapped, &unmapped);
        if (result.errorCode != 0) {
            return refused(result);
        }
        printf("%llu %llu\n", (unsigned long long)mapped, (unsigned long long)unmapped);
        return 0;
    }
    return fail("usage: pack | compress | cells | mapped (see the head of this file)");
}
