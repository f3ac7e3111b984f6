/*
 * pgrc_readslist_ord.h -- C ABI of libpgrc_rlist_ord.so: the order-preserving mode (-o) of a pseudogenome's reads list on
 * MI355X.  The lists, matchers and read sets are the objects of pgrc_readslist.h, pgrc_match.h and pgrc_readsets.h, made by
 * libpgrc_match.so; this library holds the same objects' code and four more entry points, and a handle made by one library is
 * plain memory to the other (as with libpgrc_verify.so, pgrc_verify.h).  Link it in libpgrc_match.so's place, or beside it.
 *
 * Drop-in boundary: mapReadsIntoPg with -o calls exportMatchesInOriginalOrder (matching/ReadsMatchers.cpp:597-675) instead of
 * exportMatchesInPgOrder; its archive holds neither rlOff nor rlOrgIdx (compressedBuild(.., ignoreOffDest = true)); and the
 * single-file mode writes orgIdx2PgPos itself, narrowed to 4 or 8 bytes (compressReadsPgPositions with singleFileMode).  The
 * paired mode's positions stay pgrc_rlist_pair_positions, the decoder's side pgrc_decode_set_order_positions (pgrc_decode.h).
 * Conventions as in pgrc_readslist.h.  DESIGN.md 4.20.
 */
#ifndef PGRC_READSLIST_ORD_H
#define PGRC_READSLIST_ORD_H

#include "pgrc_readslist.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t struct_size;            /* sizeof(pgrc_rlist_export_org_args) */
    int32_t pair_file_mode;          /* as pgrc_export_original_order_args: all even indexes first, then all odd ones */
    const uint32_t *read_org_idx;    /* host: the original index of every read of the matcher, */
    pgrc_rsets *sets;                /* or: SumOfMappings of the LQ and the N mapping of these sets, read on the device as
                                      * pgrc_rlist_export_args has it; never both, and one of them if the matcher has reads */
    uint64_t reads_total_count;      /* IndexesMapping::getReadsTotalCount() */
    int32_t rev_compl_pair_file;
    int32_t byte_per_read_length;
} pgrc_rlist_export_org_args;
/* exportMatchesInOriginalOrder (pgrc_match_export_original_order) with the result left in `list`: one entry per original index,
 * a filler for an index no read of the matcher carries, none for an index an unmatched read carries.  What `list` held is not
 * read (the reference reads the old list there only for orgIdx2PgPos, which is pgrc_rlist_positions' part: the HQ list stays
 * in an object of its own) and is replaced: off holds the entries' own positions cut to 16 bits (cut to off_width on the way
 * out), org_idx, RC flags and mismatch streams are the host call's, last_pos is 0 as there, off_width 1 or 2 as
 * byte_per_read_length says.  Refuses everything pgrc_match_export_original_order refuses (an index at or above the total, two
 * reads with one index, too many indexes, no run), and with PGRC_E_PARAM a matcher on another device or on several, sets on
 * another device or of another count, both forms of the indexes or (for a matcher with reads) none, 2^32 entries or
 * mismatches. */
int pgrc_rlist_export_original_order(pgrc_rlist *list, pgrc_match_ctx *matcher, const pgrc_rlist_export_org_args *args);

/* What compressedBuild(.., ignoreOffDest = true) hands to its coders in the order-preserving mode
 * (SeparatedPseudoGenomePersistence.cpp:905-952): rlRevComp and the archive form of the mismatch streams in one block by one
 * copy, neither rlOff nor rlOrgIdx.  out->off and out->org_idx are NULL, out->rev_comp is the START OF THE BLOCK; the rest as
 * pgrc_rlist_archive_encode fills it, and pgrc_rlist_archive_free gives the block back.  Refuses what that call refuses, and
 * with PGRC_E_STATE a list without RC flags or without mismatch streams. */
int pgrc_rlist_archive_encode_ord(pgrc_rlist *list, int32_t fast_level, pgrc_rlist_archive *out);

typedef struct {
    uint32_t struct_size;            /* sizeof(pgrc_rlist_positions_out) */
    uint32_t pos_width;              /* W: 4 or 8 */
    uint64_t n_total;                /* T */
    const void *positions;           /* orgIdx2PgPos: T positions of W bytes; the start of the block */
    uint64_t block_bytes;            /* the bytes the one copy brought down */
    void *block;
} pgrc_rlist_positions_out;
/* orgIdx2PgPos of the order-preserving single-file mode, as compressReadsPgPositions writes it with singleFileMode
 * (SeparatedPseudoGenomePersistence.cpp:453-462): built on the device exactly as pgrc_rlist_pair_positions builds it (the
 * same arguments, proof of "every index exactly once" and refusals; n_total may be odd here), narrowed to pos_width bytes
 * there and brought down by one copy into one block of page-locked host memory that pgrc_rlist_positions_free gives back.
 * Works on the HQ list's handle. */
int pgrc_rlist_positions(const pgrc_rlist_pairpos_args *args, pgrc_rlist_positions_out *out);
void pgrc_rlist_positions_free(pgrc_rlist_positions_out *out);     /* clears the struct */

#ifdef __cplusplus
}
#endif
#endif /* PGRC_READSLIST_ORD_H */
