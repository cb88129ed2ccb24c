/* tests/golden/fragment_length_driver.c -- command-line driver that tests/golden/make_golden_fragment_length.py links
 * against the REFERENCE's compiled counter (its native/ccounts_backend.c) and its vendored htslib.  This file is this
 * project's own: it only calls the reference's public C entry points and htslib's API, and prints what they return.
 *
 *   driver sam2bam IN.sam OUT.bam                    SAM text -> BAM + index
 *   driver dump BAM CONTIG OUT.txt                   "pos end isize flag mapq mate_same qlen" per record of CONTIG, file order
 *                                                    (qlen: core.l_qseq, or the CIGAR's query length when l_qseq <= 0)
 *   driver paired BAM MAX_READS                      prints 0 / 1 of ccounts_isPairedEnd
 *   driver readlen BAM MIN_READS MAX_ITERATIONS FLAG_EXCLUDE
 *                                                    prints the value of ccounts_getReadLength, or "ERROR <message>"
 *   driver mapped BAM [EXCLUDED_CONTIG ...]          prints "mapped unmapped" of ccounts_getMappedReadCount (coverage mode)
 *   driver fraglen BAM FLAG_EXCLUDE MAX_ITERATIONS MAX_INSERT BLOCK_SIZE ROLLING_CHUNK LAG_STEP EARLY_EXIT FALLBACK
 *                                                    prints the value of ccounts_getFragmentLength */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <htslib/hts.h>
#include <htslib/sam.h>

#include "ccounts_backend.h"

static int fail(const char *what)
{
    fprintf(stderr, "fragment_length_driver: %s\n", what);
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
        long long qlen = (long long)record->core.l_qseq;
        if (qlen <= 0 && record->core.n_cigar > 0) {
            qlen = (long long)bam_cigar2qlen((int)record->core.n_cigar, bam_get_cigar(record));
        }
        fprintf(out, "%lld %lld %lld %u %u %d %lld\n", (long long)record->core.pos, (long long)bam_endpos(record),
                (long long)record->core.isize, (unsigned)record->core.flag, (unsigned)record->core.qual,
                record->core.mtid == record->core.tid ? 1 : 0, qlen);
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
    if (argc == 4 && strcmp(argv[1], "paired") == 0) {
        ccounts_sourceConfig config = source_of(argv[2]);
        int paired = 0;
        ccounts_result result = ccounts_isPairedEnd(&config, 1, atoi(argv[3]), &paired);
        if (result.errorCode != 0) {
            return fail(result.errorMessage);
        }
        printf("%d\n", paired);
        return 0;
    }
    if (argc == 6 && strcmp(argv[1], "readlen") == 0) {
        ccounts_sourceConfig config = source_of(argv[2]);
        uint32_t length = 0;
        ccounts_result result = ccounts_getReadLength(&config, 1, atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), &length);
        if (result.errorCode != 0) {
            printf("ERROR %s\n", result.errorMessage);
        } else {
            printf("%u\n", (unsigned)length);
        }
        return 0;
    }
    if (argc >= 3 && strcmp(argv[1], "mapped") == 0) {
        ccounts_sourceConfig config = source_of(argv[2]);
        uint64_t mapped = 0, unmapped = 0;
        ccounts_result result = ccounts_getMappedReadCount(&config, 1, (const char *const *)(argv + 3), argc - 3,
                                                           (uint8_t)ccounts_countModeCoverage, 0, &mapped, &unmapped);
        if (result.errorCode != 0) {
            return fail(result.errorMessage);
        }
        printf("%llu %llu\n", (unsigned long long)mapped, (unsigned long long)unmapped);
        return 0;
    }
    if (argc == 11 && strcmp(argv[1], "fraglen") == 0) {
        ccounts_sourceConfig config = source_of(argv[2]);
        uint32_t length = 0;
        ccounts_result result = ccounts_getFragmentLength(&config, 1, atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]),
                                                          atoi(argv[7]), atoi(argv[8]), atoi(argv[9]), atoi(argv[10]), &length);
        if (result.errorCode != 0) {
            return fail(result.errorMessage);
        }
        printf("%u\n", (unsigned)length);
        return 0;
    }
    return fail("usage: sam2bam | dump | paired | readlen | mapped | fraglen (see the head of this file)");
}
