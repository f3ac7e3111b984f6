/*
 * pgrc_readsets.h -- C ABI of libpgrc_match.so, part 8: the divided read sets of the encoder, kept on MI355X between its
 * stages.
 *
 * Drop-in boundary: the DividedPCLReadsSets object (readsset/DividedPCLReadsSets.{h,cpp}): the packed HQ, LQ and N sets
 * (PackedConstantLengthReadsSet) and the two index mappings (VectorMapping), and the four edits the encoder makes between its
 * stages:
 *   moveLqReadsFromHqReadsSetsToLqReadsSets   (:145-197)  after getHQReads: the HQ reads that are not overlapped on both sides
 *                                                         are merged into the LQ set and its mapping, the HQ set is compacted
 *   generateHqReadsIndexesMapping             (:199-216)  the original indexes of the HQ reads: those in neither mapping
 *   removeReadsFromLqReadsSet                 (:218-230)  after mapReadsIntoPg (pgrc-encoder.cpp:367-372): the LQ and the N set
 *   removeReadsFromNReadsSet                  (:233-246)  and their mappings compacted by the matcher's "mapped" flags
 * The reference walks all reads in a serial loop with a copyRead per row.  Here the edits work on the original indexes: one
 * class byte per index (0 HQ, 1 LQ, 2 N, 3 moved), exclusive counts of the classes, one descriptor per output row and one
 * kernel that moves the rows.  The sets are filled from the divider (pgrc_reads.h), searched by the overlap
 * search (pgrc_overlap.h) and handed to the matcher (pgrc_match.h) where they lie: no row and no per-read flag crosses the link.
 *
 * A mapping holds count + 1 entries: the original indexes of the set's reads, strictly ascending, and the guard
 * readsTotalCount behind them (VectorMapping's last element).
 *
 * Same conventions as pgrc_overlap.h: 0 = success, PGRC_E_* otherwise; struct sizes are checked; host buffers stay the caller's;
 * no CPU fallback -- without a HIP device pgrc_rsets_create fails with PGRC_E_NO_DEVICE.  A call that returns PGRC_E_PARAM or
 * PGRC_E_STATE leaves the object as it was, and usable: every edit writes new buffers that replace the old ones only when the
 * call succeeds (for the length of a call one set's memory is held twice).
 *   PGRC_E_PARAM   a NULL pointer, a wrong struct_size or `which`; a mapping that does not ascend strictly, an index at or above
 *                  the reads' total count, an index in both mappings, an HQ count that is not total - LQ - N; a move with
 *                  n_reads_lq set (the reference exits there: the alphabets differ); more than 2^32 - 2 reads; a context of
 *                  another device, read length or shape than the call needs
 *   PGRC_E_STATE   an edit or hand-over before pgrc_rsets_finish, an append after it, an edit or hand-over on a disposed set
 */
#ifndef PGRC_READSETS_H
#define PGRC_READSETS_H

#include <stddef.h>
#include <stdint.h>

#include "pgrc_match.h"
#include "pgrc_overlap.h"
#include "pgrc_reads.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgrc_rsets pgrc_rsets;

#define PGRC_RSETS_HQ 0
#define PGRC_RSETS_LQ 1
#define PGRC_RSETS_N 2

typedef struct {
    uint32_t struct_size;            /* sizeof(pgrc_rsets_params) */
    uint32_t read_len;               /* constant read length, 1..255 */
    int32_t separate_n_reads_set;    /* DividedPCLReadsSets' constructor arguments (:10-21): they fix the three alphabets */
    int32_t n_reads_lq;
    int32_t device;                  /* HIP device, -1 = the current one */
} pgrc_rsets_params;

typedef struct {
    uint32_t struct_size;            /* sizeof(pgrc_rsets_info) */
    uint32_t finished;               /* pgrc_rsets_finish has succeeded */
    uint64_t reads_total_count;      /* A: the records appended (fixed by finish) */
    uint64_t count[3];               /* reads of the HQ, LQ and N set */
    uint32_t symbols[3];             /* 4 = "ACGT", 5 = "ACGNT", 0 = the set does not exist */
    uint32_t row_bytes[3];           /* PackedConstantLengthReadsSet::packedLength */
    uint32_t disposed[3];            /* dispose{Hq,Lq,N}ReadsSet has been called */
    uint32_t reserved;
} pgrc_rsets_info;

typedef struct {
    uint32_t struct_size;            /* sizeof(pgrc_rsets_timing) */
    uint32_t edit;                   /* the last edit: 1 move, 2 remove, 3 HQ mapping */
    float ms_checks_device;          /* device time: the classes, the checks of the mappings, the counts (scans) */
    float ms_desc_device;            /* device time: the descriptors and the new mappings */
    float ms_rows_device;            /* device time: the row mover */
    float ms_call;                   /* host wall time of the call */
    uint64_t rows_moved;             /* output rows the mover wrote */
    uint64_t bytes_moved;            /* ... and their bytes */
} pgrc_rsets_timing;

int pgrc_rsets_create(const pgrc_rsets_params *params, pgrc_rsets **out);
void pgrc_rsets_destroy(pgrc_rsets *sets);
const char *pgrc_rsets_last_error(const pgrc_rsets *sets);      /* NULL: the last failed create of this thread */

/* One batch as pgrc_divider_run* returns it (host arrays): its rows are appended to the three sets, its batch-local indexes,
 * plus the records appended so far, to the two mappings.  n_records = records of the batch (n_hq + n_lq + n_n). */
int pgrc_rsets_append(pgrc_rsets *sets, const pgrc_divided_reads *batch, uint64_t n_records);
/* The same from the divider's last run, copied on the device.  The divider has this object's device, read length and
 * constructor arguments, or PGRC_E_PARAM; PGRC_E_STATE if its last run failed or there was none. */
int pgrc_rsets_append_divider(pgrc_rsets *sets, pgrc_divider *divider);
/* Fixes readsTotalCount, writes the guards and checks the mappings as a whole. */
int pgrc_rsets_finish(pgrc_rsets *sets);

/* (pgrc_rsets_info is the struct's name, which C does not let a function share) */
int pgrc_rsets_get_info(pgrc_rsets *sets, pgrc_rsets_info *out);
/* rows [first, first + n) of set `which` (PGRC_RSETS_*): n * row_bytes bytes */
int pgrc_rsets_get_rows(pgrc_rsets *sets, int32_t which, uint64_t first, uint64_t n, uint8_t *out);
/* count + 1 entries, the guard last.  which = PGRC_RSETS_HQ: generateHqReadsIndexesMapping, the indexes in neither mapping:
 * reads_total_count - count[LQ] - count[N] + 1 entries.  That is count[HQ] + 1 until a removal; the reads a removal takes out
 * of the LQ and N sets are in neither mapping afterwards, as in the reference, though the HQ set does not hold them. */
int pgrc_rsets_get_mapping(pgrc_rsets *sets, int32_t which, uint32_t *out);
/* dispose{Hq,Lq,N}ReadsSet: the set's rows (and mapping) are given back; every later use of the set is PGRC_E_STATE */
int pgrc_rsets_dispose(pgrc_rsets *sets, int32_t which);

/* moveLqReadsFromHqReadsSetsToLqReadsSets: is_hq holds one byte per HQ row (isReadHqInHqReadsSet), in host memory or, with
 * flags_on_device != 0, in memory of the object's device.  Sets of 2^31 rows or more are PGRC_E_PARAM. */
int pgrc_rsets_move_lq(pgrc_rsets *sets, const uint8_t *is_hq, int32_t flags_on_device);
/* The same with the flags of getBothSidesOverlappedReads taken on the device from the overlap context's last run.  That run was
 * made by pgrc_rsets_overlap on this object's HQ set, and the set is unedited since: PGRC_E_STATE otherwise. */
int pgrc_rsets_move_by_overlap(pgrc_rsets *sets, pgrc_ovl_ctx *ovl);
/* removeReadsFromLqReadsSet, then removeReadsFromNReadsSet(flags, nBegIdx = the LQ count before the removal): is_mapped holds
 * LQ count + N count bytes, the LQ set's first. */
int pgrc_rsets_remove(pgrc_rsets *sets, const uint8_t *is_mapped, int32_t flags_on_device);
/* The same with flag = (pos != PGRC_NOT_MATCHED_POS), taken on the device from the matcher's result array.  A single-device
 * context on this object's device whose read count is LQ count + N count, or PGRC_E_PARAM. */
int pgrc_rsets_remove_matched(pgrc_rsets *sets, pgrc_match_ctx *matcher);

/* pgrc_ovl_run with the rows of set `which` taken on the device (read_len, symbols, n_reads and packed_rows come from the set).
 * Afterwards the overlap context is exactly as after a pgrc_ovl_run on the same rows from the host. */
int pgrc_rsets_overlap(pgrc_rsets *sets, int32_t which, pgrc_ovl_ctx *ovl, double stop_coef, uint32_t overlap_width,
                       const uint32_t *sorted_order, pgrc_ovl_result *out);
/* What SumOfConstantLengthReadsSets presents to the matcher (pgrc-encoder.cpp:349-352): pgrc_match_begin_reads(LQ + N), the LQ
 * rows and the N rows appended with their alphabets from the device, pgrc_match_end_reads.  A single-device, non-streamed
 * context of this object's device and read length, or PGRC_E_PARAM. */
int pgrc_rsets_to_matcher(pgrc_rsets *sets, pgrc_match_ctx *matcher);

/* of the last successful edit (move, remove, get_mapping(HQ)); PGRC_E_STATE before one */
int pgrc_rsets_get_timing(pgrc_rsets *sets, pgrc_rsets_timing *out);

#ifdef __cplusplus
}
#endif
#endif /* PGRC_READSETS_H */
