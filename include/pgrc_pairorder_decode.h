/*
 * pgrc_pairorder_decode.h -- C ABI of libpgrc_match.so, part of pgrc_decode.h (which includes it at its end; include that
 * header): the decoder of the pair-order coding of the paired mode that does not preserve the order, on MI355X.  The
 * coding, its forms and pgrc_pairorder_streams are described in pgrc_decode.h, "The pair-order coding"; the algorithm in
 * DESIGN.md 4.11.
 */
#ifndef PGRC_PAIRORDER_DECODE_H
#define PGRC_PAIRORDER_DECODE_H

#ifndef PGRC_DECODE_H
#error "include pgrc_decode.h"
#endif

/* decompressReadsOrder: streams as pgrc_pairorder_encode describes them (any of the four forms; host pointers);
 * rl_idx_order: T uint32, the reference's rlIdxOrder.  By form:
 *   COMPLETE_SINGLE_FILE  rev itself, a copy
 *   IGNORE                the landed pairs: [2k] = the base of pair k (the k-th entry no earlier pair has marked), [2k+1] =
 *                         its mate, the base plus the pair's decoded offset
 *   FILE_FLAGS            the landed pairs, pair k swapped iff its file flag is non-zero: off_base_file_flag[near pairs
 *                         before k] for a near pair, nonoff_base_file_flag[far pairs before k] otherwise
 *   COMPLETE              [2p] = pe[r], [2p+1] = pe[r ^ 1] with r = pair_base_org_idx[p] and pe the landed pairs (the
 *                         reference's backwards in-place loop, :420-424, computes this gather)
 * The offsets of all pairs are flag scans and one segmented sum (the chain above); the landing walks the entries in words
 * of 64 -- a word's marks settle by a relaxation of at most 64 rounds, marks that reach further travel in a bit ring of
 * 4 * PGRC_PAIRORDER_DECODE_BATCH entries in LDS, or, from 3 * PGRC_PAIRORDER_DECODE_BATCH entries on, in a bitmap in
 * device memory that is merged into the ring batch by batch.
 * PGRC_E_PARAM, where the reference would read past a vector or write out of bounds -- the context stays usable and
 * rl_idx_order is not written: n_total odd or 2^32 or more; an unknown form; a NULL stream with a non-zero count; a stream
 * that the form needs but is absent; non-zero flags in off8_flag != n_off8, or its zeros != n_delta_flag; non-zero flags in
 * delta8_flag != n_delta8, or its zeros != n_full; a decoded offset below 1; a mate at entry T or beyond; two pairs landing
 * on one entry, or the entries running out before the pairs do (the landed array is not a permutation of [0, T));
 * COMPLETE: a pair_base_org_idx value of T or more. */
#define PGRC_PAIRORDER_DECODE_BATCH 16384u  /* entries of one batch of the landing */
int pgrc_pairorder_decode(pgrc_decode_ctx *ctx, const pgrc_pairorder_streams *streams, uint32_t *rl_idx_order);

/* What pgrc_decode_set_order does for mode = PGRC_DECODE_PE, with rlIdxOrder decoded on the device straight into the
 * context's order: the array never exists on the host.  Every check of pgrc_decode_set_order runs on the decoded
 * order; after any failure the context has no order. */
int pgrc_decode_set_order_pair_order_streams(pgrc_decode_ctx *ctx, const pgrc_pairorder_streams *streams,
                                             int32_t rev_compl_pair_file);

typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_pairorder_decode_timing) */
    int32_t form;
    float ms_upload;                /* host wall time until the streams were queued for the device */
    float ms_chain_device;          /* device time: the flag scans and the segmented sum that gives every pair its offset */
    float ms_landing_device;        /* device time: the sweep (and the clearing of its bitmap) */
    float ms_tail_device;           /* device time: the form's tail (the file-flag swap, the pair_base_org_idx gather) */
    float ms_check_device;          /* device time: the permutation check of the landed array */
    float ms_download;              /* host wall time of the copy down (0 for set_order_pair_order_streams) */
    float ms_call;                  /* host wall time of the whole call (of set_order_pair_order_streams: its checks included) */
    uint64_t bytes_up, bytes_down;
    uint64_t n_near, n_delta, n_full;       /* pairs by kind (0 with COMPLETE_SINGLE_FILE) */
    uint64_t landing_words;         /* words of 64 entries the sweep settled */
    uint64_t landing_rounds;        /* relaxation rounds over all words: rounds / words is what the input cost */
} pgrc_pairorder_decode_timing;
/* of the context's last successful pgrc_pairorder_decode or pgrc_decode_set_order_pair_order_streams */
int pgrc_pairorder_get_decode_timing(pgrc_decode_ctx *ctx, pgrc_pairorder_decode_timing *out);

#endif /* PGRC_PAIRORDER_DECODE_H */
