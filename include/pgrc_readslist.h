/*
 * pgrc_readslist.h -- C ABI of libpgrc_match.so, part 9: a pseudogenome's reads list, kept on MI355X from the assembly to the
 * archive.
 *
 * Drop-in boundary: the object the second half of the encoder works on -- the reads list of a SeparatedPseudoGenome (off,
 * orgIdx, revComp and the mismatch streams of ExtendedReadsListWithConstantAccessOption / SeparatedPseudoGenomeOutputBuilder)
 * -- between runHQPgGeneration and compressReadsOrder (pgrc/pgrc-encoder.cpp):
 *   filled by     the assembly (pgrc_assemble.h) with applyIndexesMapping read from the divided read sets (pgrc_readsets.h);
 *                 exportMatchesInPgOrder (pgrc_match.h), which merges the matched LQ and N reads into the HQ list
 *   consumed by   compressedBuild's hand-over to the coders (the archive form of pgrc_decode.h), compressReadsOrder (the pair
 *                 order of the paired mode that does not keep the order) and compressReadsPgPositions over orgIdx2PgPos (the
 *                 pair positions of the mode that does)
 * No list array crosses the link unless the archive needs it: what comes down is the archive block of
 * pgrc_rlist_archive_encode and the pair streams.  The order-preserving mode's own calls are in pgrc_readslist_ord.h.
 * DESIGN.md 4.20.
 *
 * The list holds n_entries offsets (16 bits each on the device, written in off_width bytes), n_entries original indexes,
 * optionally n_entries RC flags, optionally the mismatch streams (a count per entry, n_mismatches codes, n_mismatches offsets
 * coded backwards from the read end in off_width bytes), and last_pos, the position of its last entry.
 *
 * Same conventions as pgrc_readsets.h: 0 = success, PGRC_E_* otherwise; struct sizes are checked; host buffers stay the
 * caller's; no CPU fallback -- without a HIP device pgrc_rlist_create fails with PGRC_E_NO_DEVICE.  A call that is refused
 * leaves the object as it was, and usable: every producer builds the new content beside the old one and swaps it in on success.
 * Entries and mismatches are below 2^32.  Every call is complete on return.
 */
#ifndef PGRC_READSLIST_H
#define PGRC_READSLIST_H

#include <stddef.h>
#include <stdint.h>

#include "pgrc_assemble.h"
#include "pgrc_decode.h"
#include "pgrc_match.h"
#include "pgrc_readsets.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgrc_rlist pgrc_rlist;

typedef struct {
    uint32_t struct_size;            /* sizeof(pgrc_rlist_info) */
    uint32_t off_width;              /* bytes of an offset on output: 1 (PgHelpers::bytePerReadLengthMode) or 2 */
    uint64_t n_entries;
    uint64_t n_mismatches;
    uint64_t last_pos;               /* the position of the last entry (the builder's lastWrittenPos) */
    uint32_t has_rev_comp;
    uint32_t has_mismatches;         /* the list carries mismatch streams (also where n_mismatches is 0) */
} pgrc_rlist_info;

/* the last successful call: */
enum {
    PGRC_RLIST_SET_HOST = 1,
    PGRC_RLIST_FROM_ASSEMBLY = 2,
    PGRC_RLIST_EXPORT = 3,
    PGRC_RLIST_DOWNLOAD = 4,
    PGRC_RLIST_ARCHIVE = 5,
    PGRC_RLIST_PAIR_ORDER = 6,
    PGRC_RLIST_PAIR_POSITIONS = 7,
    PGRC_RLIST_EXPORT_ORIGINAL = 8,
    PGRC_RLIST_POSITIONS = 9         /* (8 and 9: pgrc_readslist_ord.h; pgrc_rlist_archive_encode_ord reports PGRC_RLIST_ARCHIVE) */
};

typedef struct {
    uint32_t struct_size;            /* sizeof(pgrc_rlist_timing) */
    uint32_t call;                   /* PGRC_RLIST_* */
    float ms_fetch_device;           /* device time: the list's arrays taken from their source (device copies, the mapping gather,
                                      * the joined feed, the scans and scatters of the positions) */
    float ms_build_device;           /* device time: the stage itself (the export's merge, the archive form, the pair coding) */
    float ms_pack_device;            /* device time: the narrowing of off and the copies into the list or the archive block */
    float ms_call;                   /* host wall time of the call */
    uint64_t bytes_up;               /* list arrays and streams that crossed the link; words of checks and counts are not counted */
    uint64_t bytes_down;
    uint64_t bytes_device_copy;      /* bytes written by device-to-device copies of list arrays */
} pgrc_rlist_timing;

int pgrc_rlist_create(int32_t device, pgrc_rlist **out);       /* device: HIP device, -1 = the current one */
void pgrc_rlist_destroy(pgrc_rlist *list);
const char *pgrc_rlist_last_error(const pgrc_rlist *list);     /* NULL: the last failed create of this thread */
int pgrc_rlist_get_info(pgrc_rlist *list, pgrc_rlist_info *out);
/* of the last successful call on this object (pgrc_rlist_pair_order and pgrc_rlist_pair_positions: on their first list);
 * PGRC_E_STATE before one */
int pgrc_rlist_get_timing(pgrc_rlist *list, pgrc_rlist_timing *out);

/* ---- producers ---- */
/* The list from host arrays, in the form pgrc_match_export_pg_order returns: in->off holds n_entries offsets of in->off_width
 * (1 or 2) bytes, in->rev_comp may be NULL, and in->mis_cnt, in->mis_sym, in->mis_rev_off are all present (also where they
 * hold no element) or all NULL.
 * PGRC_E_PARAM: 2^32 entries or mismatches or more, off_width not 1 or 2, a NULL array with a non-zero count, one or two of the
 * three mismatch streams, n_mismatches that is not the sum of the counts (n_mismatches != 0 without the streams). */
int pgrc_rlist_set_host(pgrc_rlist *list, const pgrc_export_streams *in);

/* The reads list of the assembly context's last successful run (pgrc_asm_run, pgrc_ovl_assemble), copied on the device: off,
 * orgIdx, no RC flags, no mismatches, last_pos = pg_len - read_len, off_width 1.  With sets != NULL applyIndexesMapping runs
 * on the device, org_idx[j] = mapping[org_idx[j]], the mapping read from the read sets where it lies: `which` = PGRC_RSETS_LQ
 * or PGRC_RSETS_N is that set's mapping, PGRC_RSETS_HQ generateHqReadsIndexesMapping (the entries pgrc_rsets_get_mapping
 * returns).  sets == NULL: the indexes as the run left them.
 * PGRC_E_PARAM: a context or sets on another device; an index at or above the mapping's count (found before anything of the
 * object changes).  PGRC_E_STATE: no successful run; a run that applied a host mapping together with sets != NULL. */
int pgrc_rlist_from_assembly(pgrc_rlist *list, pgrc_asm_ctx *asm_ctx, pgrc_rsets *sets, int32_t which);

/* pgrc_ovl_assemble (without an index mapping) followed by pgrc_rlist_from_assembly, with the assembly's copy of the reads list
 * to the host left out: no list byte comes down.  *res holds the run's numbers; its org_idx and off are NULL and it needs no
 * pgrc_asm_free_result.  Refuses what the two calls refuse; after a refusal of the second the text of the run stays installed
 * in asm_ctx and the list is what it was. */
int pgrc_rlist_from_overlap(pgrc_rlist *list, pgrc_ovl_ctx *ovl, pgrc_asm_ctx *asm_ctx, pgrc_rsets *sets, int32_t which,
                            pgrc_asm_result *res);

typedef struct {
    uint32_t struct_size;            /* sizeof(pgrc_rlist_export_args) */
    int32_t order_on_device;         /* as pgrc_export_pg_order_args */
    const uint32_t *order;           /* n_matched read indexes (host) */
    uint64_t n_matched;
    const uint32_t *read_org_idx;    /* host: the original index of every read of the matcher; NULL with sets == NULL: identity */
    pgrc_rsets *sets;                /* or: SumOfMappings of the LQ and the N mapping of these sets, read on the device (LQ count + N
                                      * count must be the matcher's read count); not together with read_org_idx */
    int32_t rev_compl_pair_file;
    int32_t byte_per_read_length;
} pgrc_rlist_export_args;
/* exportMatchesInPgOrder (pgrc_match_export_pg_order) with the old list read from `list` and the merged list left in it, with
 * RC flags and mismatch streams; off_width becomes 1 or 2 as byte_per_read_length says.  Refuses everything
 * pgrc_match_export_pg_order refuses, and with PGRC_E_PARAM a matcher on another device or on several, sets on another device
 * or of another count, both forms of the original indexes; with PGRC_E_STATE a list that already carries mismatches. */
int pgrc_rlist_export_pg_order(pgrc_rlist *list, pgrc_match_ctx *matcher, const pgrc_rlist_export_args *args);

/* ---- consumers ---- */
/* The streams exactly as pgrc_match_export_pg_order returns them (malloc'ed; pgrc_match_free_export).  A list without RC
 * flags or without mismatch streams gives zeros there, as that call does for such an old list. */
int pgrc_rlist_download(pgrc_rlist *list, pgrc_export_streams *out);

typedef struct {
    uint32_t struct_size;            /* sizeof(pgrc_rlist_archive) */
    uint32_t off_width;
    uint64_t n_entries;
    const uint8_t *off;              /* rlOff: n_entries offsets of off_width bytes; the START OF THE BLOCK */
    const uint8_t *rev_comp;         /* rlRevComp: n_entries, or NULL: the list has none */
    const uint32_t *org_idx;         /* rlOrgIdx: n_entries, or NULL: not asked for */
    uint64_t block_bytes;            /* the bytes the one copy brought down */
    void *block;
    pgrc_list_archive_streams archive;   /* as pgrc_list_archive_encode fills it, inside the same block (its `block` is NULL);
                                          * all zero for a list without mismatch streams */
} pgrc_rlist_archive;
/* What compressedBuild hands to the coders, in ONE block of page-locked host memory filled by one copy from the device:
 * rlOff, rlRevComp, rlOrgIdx if want_org_idx != 0, and the archive form of the mismatch streams (pgrc_list_archive_encode's
 * rules and refusals; it needs off_width 1).  pgrc_rlist_archive_free gives the block back.  The list stays as it is. */
int pgrc_rlist_archive_encode(pgrc_rlist *list, int32_t fast_level, int32_t want_org_idx, pgrc_rlist_archive *out);
void pgrc_rlist_archive_free(pgrc_rlist_archive *arch);        /* clears the struct */

/* compressReadsOrder (pgrc_pairorder_encode) with the original indexes of the lists HQ, LQ, N read on the device; NULL = no
 * such list.  The lists lie on one device; the call works on the first list's handle.  *out is freed by pgrc_pairorder_free. */
int pgrc_rlist_pair_order(pgrc_rlist *const lists[3], int32_t form, pgrc_pairorder_streams *out);

typedef struct {
    uint32_t struct_size;            /* sizeof(pgrc_rlist_pairpos_args) */
    uint32_t pos_width;              /* 4 or 8 */
    uint64_t n_total;                /* T = readsTotalCount, even */
    pgrc_rlist *hq;                  /* the HQ list as the assembly left it (ReadsMatchers.cpp:604-610) */
    pgrc_rlist *lq;                  /* at base hq_len (pgrc-encoder.cpp:173-178); NULL: none */
    pgrc_rlist *n;                   /* at base hq_len + lq_len (:193-198); NULL: none */
    uint64_t hq_len, lq_len;         /* the pseudogenomes' lengths */
    pgrc_match_ctx *matcher;         /* its matched reads: pos[original index] = match position (ReadsMatchers.cpp:659); NULL: none */
    const uint32_t *read_org_idx;    /* the matcher's reads' original indexes: a host array, */
    pgrc_rsets *sets;                /* or the LQ and N mappings of these sets (as pgrc_rlist_export_args) */
} pgrc_rlist_pairpos_args;
/* orgIdx2PgPos of the order-preserving paired mode, built on the device -- T elements of all ones, pos[org_idx[i]] = base + the
 * sum of off[0 .. i] for every list, the matcher's positions -- and coded by pgrc_pairpos_encode's device side without ever
 * existing on the host.  Every index in [0, T) must be written exactly once: PGRC_E_PARAM otherwise (an index of T or more, an
 * index written twice, an index never written), and for a position of 2^32 or more with pos_width 4.  Works on the HQ list's
 * handle.  *out is freed by pgrc_pairpos_free. */
int pgrc_rlist_pair_positions(const pgrc_rlist_pairpos_args *args, pgrc_pairpos_streams *out);


#ifdef __cplusplus
}
#endif
#endif /* PGRC_READSLIST_H */
