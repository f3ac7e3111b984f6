/*
 * pgrc_reads_text.h -- C ABI of libpgrc_reads_text.so (everything libpgrc_verify.so holds, and readstext.hip):
 * the two entries around pgrc_divider_run_text (pgrc_reads.h) that have no place in the older libraries, whose exported names
 * are fixed -- a library of its own, as libpgrc_verify.so and libpgrc_rlist_ord.so are.  pgrc_divider_run_text itself is in
 * every library, beside pgrc_divider_run_fastq.
 *
 * Same conventions as pgrc_verify.h.  A verifier made by pgrc_verify_begin of libpgrc_verify.so is a valid handle here, and
 * the other way round: the libraries hold the same code.
 */
#ifndef PGRC_READS_TEXT_H
#define PGRC_READS_TEXT_H

#include <stddef.h>
#include <stdint.h>

#include "pgrc_reads.h"
#include "pgrc_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the reference's choice by the first byte of the FILE (ManagedReadsSetIterator, readsset/persistance/ReadsSetPersistence.cpp:
 * 36-47): '@' -> PGRC_READS_FASTQ, '>' or ';' -> PGRC_READS_FASTA, anything else -> PGRC_READS_LINES -- an empty file too
 * (first_byte = -1, what istream::get returns there).  Of the file, not of a piece: a later piece may begin with any byte. */
int pgrc_reads_text_format(int first_byte);

/* pgrc_verify_add_fastq for any of the three text formats: its arguments with `format` (PGRC_READS_*) after the handle, the
 * contract of pgrc_divider_run_text for pieces, final_piece, consumed and pair files of unequal length, rev_compl_pair = 0.
 * PGRC_READS_FASTQ is pgrc_verify_add_fastq.  Refuses what the divider refuses: PGRC_READS_LINES with pair_text (so a job
 * of two files takes no one-read-per-line source), an unknown format, a read that is not L letters long (PGRC_E_PARAM); a
 * symbol outside ACGNT (PGRC_E_SYMBOL). */
int pgrc_verify_add_text(pgrc_verify *v, int32_t format, const char *text, uint64_t bytes, const char *pair_text, uint64_t pair_bytes,
                         int32_t final_piece, uint64_t *consumed, uint64_t *pair_consumed, uint64_t *n_records);

#ifdef __cplusplus
}
#endif
#endif /* PGRC_READS_TEXT_H */
