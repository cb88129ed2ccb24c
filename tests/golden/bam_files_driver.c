/* tests/golden/bam_files_driver.c -- command-line driver that tests/golden/make_golden_bam_files.py links against the
 * REFERENCE's vendored htslib.  This file is this project's own: it only calls htslib's API and prints what it returns.
 *
 *   driver sam2bam IN.sam OUT.bam      SAM text -> BAM (htslib writes the records, a CG tag where a CIGAR is too long)
 *   driver index BAM                   builds BAM.bai
 *   driver dumpall BAM OUT.txt         "tid pos end isize flag mapq mate_same qlen" per record of the WHOLE file, in file
 *                                      order, the records without a contig (tid -1) included; end is bam_endpos, qlen is
 *                                      core.l_qseq, or bam_cigar2qlen where l_qseq <= 0: htslib does all the decoding */
#include <stdio.h>
#include <string.h>

#include <htslib/hts.h>
#include <htslib/sam.h>

static int fail(const char *what)
{
    fprintf(stderr, "bam_files_driver: %s\n", what);
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
    return sam_close(out) < 0 ? fail("cannot finish the BAM file") : 0;
}

static int dumpall(const char *bam_path, const char *out_path)
{
    samFile *in = sam_open(bam_path, "r");
    sam_hdr_t *header = in != NULL ? sam_hdr_read(in) : NULL;
    FILE *out = fopen(out_path, "w");
    if (header == NULL || out == NULL) {
        return fail("cannot open the BAM input or the dump output");
    }
    bam1_t *record = bam_init1();
    int rc;
    while ((rc = sam_read1(in, header, record)) >= 0) {
        long long qlen = (long long)record->core.l_qseq;
        if (qlen <= 0 && record->core.n_cigar > 0) {
            qlen = (long long)bam_cigar2qlen((int)record->core.n_cigar, bam_get_cigar(record));
        }
        fprintf(out, "%d %lld %lld %lld %u %u %d %lld\n", (int)record->core.tid, (long long)record->core.pos,
                (long long)bam_endpos(record), (long long)record->core.isize, (unsigned)record->core.flag,
                (unsigned)record->core.qual, record->core.mtid == record->core.tid ? 1 : 0, qlen);
    }
    bam_destroy1(record);
    sam_hdr_destroy(header);
    sam_close(in);
    fclose(out);
    return rc < -1 ? fail("a record does not decode") : 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && strcmp(argv[1], "sam2bam") == 0) {
        return sam2bam(argv[2], argv[3]);
    }
    if (argc == 3 && strcmp(argv[1], "index") == 0) {
        return sam_index_build(argv[2], 0) < 0 ? fail("cannot build the index") : 0;
    }
    if (argc == 4 && strcmp(argv[1], "dumpall") == 0) {
        return dumpall(argv[2], argv[3]);
    }
    return fail("usage: sam2bam | index | dumpall (see the head of this file)");
}
