// readstext.hip -- the entries of include/pgrc_reads_text.h: libpgrc_reads_text.so is the product's objects, verify.hip and this
// file (the older libraries keep the names they export).  Host code only: the kernels behind these entries are divide.hip's
// (pgrc_divider_run_text) and verify.hip's.
#include "pgrc_reads_text.h"
#include "verifyctx.h"

extern "C" {

// ManagedReadsSetIterator (readsset/persistance/ReadsSetPersistence.cpp:36-47): `char firstSymbol = srcSource->get()` and a switch
int pgrc_reads_text_format(int first_byte) {
    switch (first_byte) {
    case '@': return PGRC_READS_FASTQ;
    case '>':
    case ';': return PGRC_READS_FASTA;
    default: return PGRC_READS_LINES;
    }
}

int pgrc_verify_add_text(pgrc_verify *v, int32_t format, const char *text, uint64_t bytes, const char *pair_text, uint64_t pair_bytes,
                         int32_t final_piece, uint64_t *consumed, uint64_t *pair_consumed, uint64_t *n_records) {
    return pgrc_vf_add_text(v, "add_text", format, text, bytes, pair_text, pair_bytes, final_piece, consumed, pair_consumed, n_records);
}

}   // extern "C"
