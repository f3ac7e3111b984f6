/*
 * pgrc_verify.h -- C ABI of libpgrc_verify.so (everything libpgrc_match.so holds, and verify.hip): does a
 * decode job give the source reads back?  The comparison runs on MI355X; neither the rebuilt rows nor a per-row verdict
 * crosses the link.
 *
 * The reference's decoder has this stage behind `-i src [pair]` (preparePgsForValidation / validateAllPgs /
 * validatePgsOrder, pgrc/pgrc-decoder.cpp:552-695), on top of the orgIdx dumps of a developer build.  It is not restated
 * here: the rule below is the archive's promise itself.
 *
 * A verifier works on a decode context (`job`, pgrc_decode.h) with text, lists and order set.  The job has F files
 * (pgrc_decode_row_count: SE 1, PE 2, ORD 1 or 2) of rows of L symbols.  An ITEM is row r of every file: L bytes for one
 * file, 2 L bytes for two (file 0's row, then file 1's row); the row's '\n' is not part of it.
 *   IN_ORDER   row r of every source file equals row r of the job's file.  Streams: as source rows arrive, the job's rows
 *              of the same range are made by the row kernel into a buffer of the handle (chunks of at most 64 MiB) and
 *              compared; nothing is kept.
 *   MULTISET   the source items and the job's items are the same multiset.  Both sides stay resident until finish:
 *              N * F * L bytes of source and N * F * (L + 1) bytes of rebuilt rows, and 56 bytes per item of BOTH sides for
 *              the keys, the sort and the scans (at 10^8 reads of 150 bp: 15 GB + 15.1 GB + 11.2 GB).  Every item gets a
 *              64-bit key; one stable sort of the union of both sides' keys pairs the items of equal keys in index order;
 *              every pair is then compared byte for byte.  Equal bytes are a match; different bytes under equal keys are
 *              UNDECIDED, never a match -- so ok = 1 is a proof, not a probability.  With undecided pairs the whole is
 *              repeated under the next salt of the key, three salts at the most.
 *              Among equal items the ones with the smallest indexes are matched first: of m source items and k < m decoded
 *              items that are equal, the LAST m - k source items (by item index) are the unmatched ones.
 * PGRC_VERIFY_AUTO picks IN_ORDER for an ORD job and MULTISET for SE and PE: what each archive mode promises to keep.
 *
 * Same conventions as pgrc_readslist.h: 0 = success, PGRC_E_* otherwise; struct sizes are checked; host buffers stay the
 * caller's; no CPU fallback.  A call that is refused (PGRC_E_PARAM, PGRC_E_STATE) leaves the handle usable and as it was.
 * Out of scope: archives written with the pair order ignored, several devices, qualities and identifiers.
 */
#ifndef PGRC_VERIFY_H
#define PGRC_VERIFY_H

#include <stddef.h>
#include <stdint.h>

#include "pgrc_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgrc_verify pgrc_verify;
enum { PGRC_VERIFY_AUTO = 0, PGRC_VERIFY_IN_ORDER = 1, PGRC_VERIFY_MULTISET = 2 };
#define PGRC_VERIFY_MAX_ITEMS 0x7FFFF800ull     /* MULTISET: items of one side (the union sort's record limit) */

/* `job` is borrowed: it must outlive the verifier, and no other call may change its text, lists or order meanwhile.
 * PGRC_E_STATE: a job without an order.  PGRC_E_PARAM: an unknown kind; MULTISET on a job of more than
 * PGRC_VERIFY_MAX_ITEMS items. */
int pgrc_verify_begin(pgrc_decode_ctx *job, int32_t kind, pgrc_verify **out);
void pgrc_verify_end(pgrc_verify *v);
const char *pgrc_verify_last_error(const pgrc_verify *v);   /* NULL: the last failed pgrc_verify_begin of this thread */

/* n source rows of L bytes (no newline) of file `file`, in source order, appended to what the file has so far; the files
 * may run ahead of one another.  Page-locked memory is read by the copy engine where it is, other memory goes through the
 * handle's staging buffers.  PGRC_E_PARAM: file >= F; rows NULL with n > 0; MULTISET: more than PGRC_VERIFY_MAX_ITEMS rows. */
int pgrc_verify_add_rows(pgrc_verify *v, uint32_t file, const char *rows, uint64_t n);

/* The same from FASTQ text, under the contract of pgrc_divider_run_fastq (pgrc_reads.h) for pieces, final_piece, consumed
 * and pair files of unequal length, with rev_compl_pair = 0: the decoder's output is the source as it was.  pair_text is
 * the second file's piece: NULL for a job of one file, needed (pair_bytes may be 0) for a job of two.  *n_records = records
 * taken, the files in turn.  Refuses what the divider refuses (a read that is not L letters long, text that ends inside a
 * record: PGRC_E_PARAM; a symbol outside ACGNT: PGRC_E_SYMBOL).
 * A FASTA or one-read-per-line source goes through pgrc_verify_add_text (pgrc_reads_text.h, libpgrc_reads_text.so: this
 * library's seven names stay seven), which takes a handle of this library as it is. */
int pgrc_verify_add_fastq(pgrc_verify *v, const char *text, uint64_t bytes, const char *pair_text, uint64_t pair_bytes,
                          int32_t final_piece, uint64_t *consumed, uint64_t *pair_consumed, uint64_t *n_records);

typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_verify_result) */
    int32_t kind;                   /* PGRC_VERIFY_IN_ORDER or PGRC_VERIFY_MULTISET */
    int32_t ok;                     /* 1 iff the counts agree per file and every failure counter below is 0 */
    uint32_t salts_used;            /* MULTISET: 1 .. 3 (0 when neither side has an item); IN_ORDER: 0 */
    uint64_t n_source[2], n_decoded[2];     /* rows per file */
    /* IN_ORDER: over rows [0, min(n_source, n_decoded)) of each file.  mismatched_rows sums the files; the first mismatch
     * is the one with the smallest row, of two in the same row the one in file 0 (UINT32_MAX / UINT64_MAX: none) */
    uint64_t mismatched_rows;
    uint32_t first_mismatch_file;
    uint64_t first_mismatch_row;
    /* MULTISET, of the last salt tried.  The source has min over the files of n_source items (rows of a longer file beyond
     * that are counted in n_source and otherwise ignored), the job min over the files of n_decoded.  undecided counts
     * pairs; its items are in neither unmatched count */
    uint64_t source_unmatched, decoded_unmatched, undecided;
    uint64_t first_source_unmatched, first_decoded_unmatched;   /* smallest item index; UINT64_MAX: none */
} pgrc_verify_result;
/* Once; afterwards only pgrc_verify_get_timing and pgrc_verify_end are valid (PGRC_E_STATE otherwise).  A refused finish
 * (a wrong struct_size) is not counted. */
int pgrc_verify_finish(pgrc_verify *v, pgrc_verify_result *out);

typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_verify_timing) */
    uint32_t salts_used;
    float ms_upload;                /* host wall time of the add_rows calls (IN_ORDER: their row kernels and compares included) */
    float ms_fastq;                 /* host wall time of the add_fastq calls */
    float ms_fastq_parse_device;    /* ... of which the divider's upload and parse */
    float ms_fastq_pack_device;     /* ... and its classification, packing and copy down: not needed here */
    float ms_rows_device;           /* device time of the row kernels */
    float ms_compare_device;        /* IN_ORDER: device time of k_vf_compare */
    float ms_hash_device;           /* MULTISET, summed over the salts: keys of both sides */
    float ms_sort_device;           /* the union sort */
    float ms_scan_device;           /* head flags, the two scans, the compaction */
    float ms_confirm_device;        /* the byte compare of the pairs */
    float ms_finish;                /* host wall time of pgrc_verify_finish */
    float ms_total;                 /* host wall time from pgrc_verify_begin to the end of pgrc_verify_finish */
    uint64_t bytes_up;              /* source bytes that went up */
    uint64_t bytes_resident;        /* device memory the handle held at finish */
} pgrc_verify_timing;
int pgrc_verify_get_timing(pgrc_verify *v, pgrc_verify_timing *out);

#ifdef __cplusplus
}
#endif
#endif /* PGRC_VERIFY_H */
