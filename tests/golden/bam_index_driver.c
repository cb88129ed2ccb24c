/* tests/golden/bam_index_driver.c -- command-line driver that tests/golden/make_golden_bam_index.py links against the
 * REFERENCE's vendored htslib.  This file is this project's own: it only calls htslib's API and prints what it returns.
 *
 *   driver dump BAM OUT.txt     loads BAM's index (BAM.bai) and writes, per reference of the header, one line
 *                                   "ref TID HAS_STAT N_MAPPED N_UNMAPPED N ORDINAL*N"
 *                               where the ordinals are the positions, in file order, of the records that
 *                               sam_itr_queryi(idx, tid, 0, length) yields, in the order it yields them; HAS_STAT is 1 where
 *                               hts_idx_get_stat answers; then one line "nocoor N" (hts_idx_get_n_no_coor) and one line
 *                               "records N" (the records of the whole file).
 * The ordinal of an iterator's record is found by reading the whole file once (sam_read1) and keeping per record its
 * refID, position, flag, template length, query length and name; the iterator's records are matched against that list
 * going forward only. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <htslib/hts.h>
#include <htslib/sam.h>

typedef struct {
    int32_t tid, flag, l_qseq;
    int64_t pos, isize;
    char name[256];
} seen_t;

static int fail(const char *what)
{
    fprintf(stderr, "bam_index_driver: %s\n", what);
    return 1;
}

static void note(seen_t *s, const bam1_t *b)
{
    memset(s, 0, sizeof(*s));
    s->tid = b->core.tid;
    s->flag = b->core.flag;
    s->l_qseq = b->core.l_qseq;
    s->pos = b->core.pos;
    s->isize = b->core.isize;
    strncpy(s->name, bam_get_qname(b), sizeof(s->name) - 1);
}

static int dump(const char *bam_path, const char *out_path)
{
    samFile *in = sam_open(bam_path, "r");
    sam_hdr_t *header = in != NULL ? sam_hdr_read(in) : NULL;
    FILE *out = fopen(out_path, "w");
    if (header == NULL || out == NULL) {
        return fail("cannot open the BAM input or the dump output");
    }
    size_t n = 0, room = 1024;
    seen_t *seen = malloc(room * sizeof(seen_t));
    bam1_t *record = bam_init1();
    int rc;
    while ((rc = sam_read1(in, header, record)) >= 0) {
        if (n == room) {
            room *= 2;
            seen = realloc(seen, room * sizeof(seen_t));
        }
        note(&seen[n++], record);
    }
    if (rc < -1 || seen == NULL) {
        return fail("the BAM file does not read to its end");
    }
    sam_close(in);
    in = sam_open(bam_path, "r");
    hts_idx_t *idx = in != NULL ? sam_index_load(in, bam_path) : NULL;
    if (idx == NULL) {
        return fail("cannot load the index");
    }
    const int n_ref = sam_hdr_nref(header);
    size_t *ordinals = malloc((n + 1) * sizeof(size_t));
    for (int tid = 0; tid < n_ref; ++tid) {
        uint64_t mapped = 0, unmapped = 0;
        const int has_stat = hts_idx_get_stat(idx, tid, &mapped, &unmapped) == 0;
        hts_itr_t *itr = sam_itr_queryi(idx, tid, 0, sam_hdr_tid2len(header, tid));
        size_t count = 0, at = 0;
        if (itr != NULL) {
            while ((rc = sam_itr_next(in, itr, record)) >= 0) {
                seen_t s;
                note(&s, record);
                while (at < n && memcmp(&seen[at], &s, sizeof(s)) != 0) {
                    ++at;
                }
                if (at == n) {
                    return fail("the iterator yields a record the file does not hold behind the one before");
                }
                ordinals[count++] = at++;
            }
            if (rc < -1) {
                return fail("the iterator fails");
            }
            hts_itr_destroy(itr);
        }
        fprintf(out, "ref %d %d %llu %llu %zu", tid, has_stat, (unsigned long long)mapped, (unsigned long long)unmapped, count);
        for (size_t k = 0; k < count; ++k) {
            fprintf(out, " %zu", ordinals[k]);
        }
        fprintf(out, "\n");
    }
    fprintf(out, "nocoor %llu\nrecords %zu\n", (unsigned long long)hts_idx_get_n_no_coor(idx), n);
    free(ordinals);
    free(seen);
    bam_destroy1(record);
    hts_idx_destroy(idx);
    sam_hdr_destroy(header);
    sam_close(in);
    return fclose(out) != 0 ? fail("cannot finish the dump") : 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && strcmp(argv[1], "dump") == 0) {
        return dump(argv[2], argv[3]);
    }
    return fail("usage: dump BAM OUT.txt");
}
