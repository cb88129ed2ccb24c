/* tests/golden/alignment_counts_driver.c -- command-line driver that tests/golden/make_golden_alignment_counts.py links
 * against the REFERENCE's compiled counter (its native/ccounts_backend.c) and its vendored htslib.  This file is this
 * project's own: it only calls the reference's public C entry points and htslib's API, and prints / stores what they return.
 *
 *   driver sam2bam IN.sam OUT.bam                      SAM text -> BAM + index
 *   driver dump BAM CONTIG OUT.txt                     "pos end isize flag mapq mate_same" per record of CONTIG, file order
 *   driver range BAM CONTIG CHROM_LEN FLAG_EXCLUDE     prints "start end" of ccounts_getChromRange
 *   driver count BAM CONTIG START END STEP LENGTH PREFILL OUT.f32 ONE_READ_PER_BIN FLAG_INCLUDE FLAG_EXCLUDE SHIFT_FWD
 *          SHIFT_REV READ_LENGTH EXTEND_BP MIN_MAPQ MIN_TEMPLATE MAX_INSERT PAIRED_END_MODE
 *                                                      LENGTH float32 counts of ccounts_countRegion (count mode coverage)
 *                                                      into a buffer that holds (i % PREFILL) before the call (0: zeros) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <htslib/hts.h>
#include <htslib/sam.h>

#include "ccounts_backend.h"

static int fail(const char *what)
{
    fprintf(stderr, "alignment_counts_driver: %s\n", what);
    return 1;
}

static int sam2bam(const char *in_path, const char *out_path)
{
    samFile *in = sam_open(in_path, "r");
    samFile *out = sam_open(out_path, "wb");
    if (in == NULL || out == NULL) {
        return fail("cannot open the SAM input or the BAM output");
    }
    sam_hdr_t *header = sam_hdr_read(in);
    if (header == NULL || sam_hdr_write(out, header) < 0) {
        return fail("cannot copy the header");
    }
    bam1_t *record = bam_init1();
    int rc;
    while ((rc = sam_read1(in, header, record)) >= 0) {
        if (sam_write1(out, header, record) < 0) {
            return fail("cannot write a record");
        }
    }
    if (rc < -1) {
        return fail("the SAM text does not parse");
    }
    bam_destroy1(record);
    sam_hdr_destroy(header);
    sam_close(in);
    if (sam_close(out) < 0) {
        return fail("cannot finish the BAM file");
    }
    return sam_index_build(out_path, 0) < 0 ? fail("cannot build the index") : 0;
}

static int dump(const char *bam_path, const char *contig, const char *out_path)
{
    samFile *in = sam_open(bam_path, "r");
    sam_hdr_t *header = in != NULL ? sam_hdr_read(in) : NULL;
    FILE *out = fopen(out_path, "w");
    if (header == NULL || out == NULL) {
        return fail("cannot open the BAM input or the dump output");
    }
    const int tid = sam_hdr_name2tid(header, contig);
    bam1_t *record = bam_init1();
    while (sam_read1(in, header, record) >= 0) {
        if (record->core.tid != tid) {
            continue;
        }
        fprintf(out, "%lld %lld %lld %u %u %d\n", (long long)record->core.pos, (long long)bam_endpos(record),
                (long long)record->core.isize, (unsigned)record->core.flag, (unsigned)record->core.qual,
                record->core.mtid == record->core.tid ? 1 : 0);
    }
    bam_destroy1(record);
    sam_hdr_destroy(header);
    sam_close(in);
    fclose(out);
    return 0;
}

static ccounts_sourceConfig source_of(const char *bam_path)
{
    ccounts_sourceConfig config;
    memset(&config, 0, sizeof(config));
    config.path = bam_path;
    config.sourceKind = ccounts_sourceKindBAM;
    return config;
}

int main(int argc, char **argv)
{
    if (argc == 4 && strcmp(argv[1], "sam2bam") == 0) {
        return sam2bam(argv[2], argv[3]);
    }
    if (argc == 5 && strcmp(argv[1], "dump") == 0) {
        return dump(argv[2], argv[3], argv[4]);
    }
    if (argc == 6 && strcmp(argv[1], "range") == 0) {
        ccounts_sourceConfig config = source_of(argv[2]);
        uint64_t start = 0, end = 0;
        ccounts_result result = ccounts_getChromRange(&config, argv[3], (uint64_t)strtoull(argv[4], NULL, 10), 1, atoi(argv[5]),
                                                      &start, &end);
        if (result.errorCode != 0) {
            return fail(result.errorMessage);
        }
        printf("%llu %llu\n", (unsigned long long)start, (unsigned long long)end);
        return 0;
    }
    if (argc == 21 && strcmp(argv[1], "count") == 0) {
        ccounts_sourceConfig config = source_of(argv[2]);
        ccounts_region region;
        ccounts_countOptions options;
        memset(&options, 0, sizeof(options));
        region.chromosome = argv[3];
        region.start = (uint32_t)strtoul(argv[4], NULL, 10);
        region.end = (uint32_t)strtoul(argv[5], NULL, 10);
        region.intervalSizeBP = (uint32_t)strtoul(argv[6], NULL, 10);
        const size_t length = (size_t)strtoull(argv[7], NULL, 10);
        const int prefill = atoi(argv[8]);
        options.countMode = (uint8_t)ccounts_countModeCoverage;
        options.oneReadPerBin = (uint8_t)(atoi(argv[10]) != 0);
        options.flagInclude = (uint16_t)atoi(argv[11]);
        options.flagExclude = (uint16_t)atoi(argv[12]);
        options.shiftForwardStrand53 = atoll(argv[13]);
        options.shiftReverseStrand53 = atoll(argv[14]);
        options.readLength = atoll(argv[15]);
        options.extendBP = atoll(argv[16]);
        options.minMappingQuality = atoll(argv[17]);
        options.minTemplateLength = atoll(argv[18]);
        options.maxInsertSize = atoll(argv[19]);
        options.pairedEndMode = atoll(argv[20]);
        float *counts = (float *)calloc(length + 1, sizeof(float));
        for (size_t i = 0; prefill > 0 && i < length; ++i) {
            counts[i] = (float)(i % (size_t)prefill);
        }
        ccounts_sourceHandle *handle = NULL;
        ccounts_result result = ccounts_openSource(&config, &handle);
        if (result.errorCode == 0) {
            result = ccounts_countRegion(handle, &region, &options, counts, length);
        }
        if (handle != NULL) {
            ccounts_closeSource(handle);
        }
        if (result.errorCode != 0) {
            return fail(result.errorMessage);
        }
        FILE *out = fopen(argv[9], "wb");
        if (out == NULL || fwrite(counts, sizeof(float), length, out) != length) {
            return fail("cannot write the counts");
        }
        fclose(out);
        free(counts);
        return 0;
    }
    return fail("usage: sam2bam | dump | range | count (see the head of this file)");
}
