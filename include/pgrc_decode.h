/*
 * pgrc_decode.h -- C ABI of libpgrc_match.so, part 3: the rebuild of the reads from the pseudogenomes and their reads
 * lists (the inverse of the export, row f1) on MI355X.
 *
 * What the reference's decoder does after loading an archive (pgrc/pgrc-decoder.cpp): it holds three separated
 * pseudogenomes -- HQ, LQ and N -- each with its reads list, and writes every read as `L` symbols plus '\n' in one of
 * three orders:
 *   SE   writeAllReadsInSEMode*  (:137-239)  every list in list order, HQ, then LQ, then N
 *   PE   writeAllReadsInPEMode*  (:241-383)  file p holds rows i = p (mod 2) of rlIdxOrder
 *   ORD  writeAllReadsInORDMode* (:385-527)  one row per original index, from orgIdx2PgPos in the JOINED text
 * Per entry (SeparatedPseudoGenome.cpp:74-120): the raw window text[pos, pos+L), reverse-complemented in place when its
 * RC flag is set (utils/helper.cpp complementsLut, N -> N), then every mismatch i sets
 * ptr[misOff[i]] = code2mismatch(ptr[misOff[i]], misSymCode[i]) (helper.cpp:353-356) under the symbol order of the
 * archive header (pgrc-decoder.cpp:731-735).  Entries are numbered HQ, then LQ, then N (rlIdx).
 *
 * Here the host hands over the joined text and the streams of every list (entropy decoding and archive parsing stay with
 * the caller) -- either reassembled per entry (pgrc_decode_add_list) or, since pgrc_decode_add_list_archive, as the archive
 * holds them: the reassembly of the mismatch streams no longer has to stay with the caller; positions and mismatch list starts are prefix scans on the device, every row
 * is an independent job of a row kernel that assembles tiles of rows in LDS, and rows come back to the host in chunks
 * copied down while the next chunk is made.  More of the decoder's stages follow further down: the restore of the matched
 * pseudogenomes, the pair-position coding of the order-preserving paired mode (with its encoder), the pair-order coding
 * of the other paired mode (with its encoder) and the archive form of a list's mismatch streams (both directions).
 *
 * Same conventions as pgrc_match.h: 0 = success, PGRC_E_* otherwise; host buffers stay the caller's (nothing is
 * borrowed beyond a call); no CPU fallback -- without a HIP device every call fails.
 */
#ifndef PGRC_DECODE_H
#define PGRC_DECODE_H

#include <stddef.h>
#include <stdint.h>

#include "pgrc_match.h"
#include "pgrc_varlen.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgrc_decode_ctx pgrc_decode_ctx;

/* 1 <= read_length <= 255 (the reads lists' uint8 read length). */
int pgrc_decode_create(uint32_t read_length, int32_t device, pgrc_decode_ctx **out);
void pgrc_decode_destroy(pgrc_decode_ctx *ctx);
const char *pgrc_decode_last_error(const pgrc_decode_ctx *ctx);   /* NULL: the last failed create of this thread */

/* The joined text HQ | LQ | N (the three pgSequences one after the other; hqPgLen and nonNPgLen are the text_base of
 * the LQ and N lists).  Any bytes, N included; kept as bytes.  Copied to the device; drops the lists and the order. */
int pgrc_decode_set_text(pgrc_decode_ctx *ctx, const char *joined, uint64_t len);

/* One reads list, as ExtendedReadsListWithConstantAccessOption holds it after loading.  Lists are added HQ, LQ, N in
 * that order (rlIdx numbers their entries one after the other).  The LQ and N lists carry no RC flags and no
 * mismatches (pgrc-decoder.cpp loadAllPgs: disableRevCompl, disableMismatches): rev_comp and mis_cnt must be NULL
 * there. */
typedef struct {
    uint32_t struct_size;       /* sizeof(pgrc_decode_list) */
    uint64_t text_base;         /* where this list's pseudogenome starts in the joined text: 0, hqPgLen, nonNPgLen */
    uint64_t n_entries;
    const void *off;            /* offset deltas (rlOff), off_width bytes each: positions are their inclusive scan
                                 * (enableConstantAccess, SeparatedExtendedReadsList.cpp:328-363) ... */
    uint32_t off_width;         /* 1 (PgHelpers::bytePerReadLengthMode) or 2 */
    const uint64_t *pos;        /* ... or, with off NULL, the absolute positions in the list's own text.  Both NULL: the
                                 * list has no positions (the HQ list of an ORD job, enableConstantAccess(.., true)) */
    const uint8_t *rev_comp;    /* n_entries RC flags; NULL = revComp disabled */
    const uint8_t *mis_cnt;     /* n_entries mismatch counts; NULL = mismatches disabled */
    const uint8_t *mis_sym;     /* sum(mis_cnt) mismatch codes */
    const void *mis_off;        /* sum(mis_cnt) mismatch offsets, mis_off_width bytes each */
    uint32_t mis_off_width;     /* 1 or 2; 0 = off_width (1 when off is NULL) */
    int32_t mis_off_rev_coded;  /* 1 = rlMisRevOff as the archive and pgrc_export_streams hold it (per entry coded
                                 * backwards from the read end, turned into offsets by convertMisRevOffsets2Offsets,
                                 * utils/helper.h:52-63); 0 = forward offsets */
    int32_t mis_sym_form;       /* 0 = the archive's exclusive code under bases_order (code2mismatch); 1 = the context
                                 * code (actual << 4) + mismatch of pgrc_export_streams, values in "ACGTN" order */
    const char *bases_order;    /* 5 symbols (archive header, reorderSymAndVal); NULL = "ACGTN" */
} pgrc_decode_list;
int pgrc_decode_add_list(pgrc_decode_ctx *ctx, const pgrc_decode_list *list);

enum { PGRC_DECODE_SE = 0, PGRC_DECODE_PE = 1, PGRC_DECODE_ORD = 2 };
typedef struct {
    uint32_t struct_size;          /* sizeof(pgrc_decode_order) */
    int32_t mode;                  /* PGRC_DECODE_SE / _PE / _ORD */
    uint64_t n_total;              /* readsTotalCount: entries of rl_idx_order (PE) or org_idx_to_pos (ORD); SE: ignored */
    const uint32_t *rl_idx_order;  /* PE: rlIdxOrder, every value below the lists' total entry count */
    const uint64_t *org_idx_to_pos;/* ORD: orgIdx2PgPos (joined-text positions; below hqPgLen = an HQ entry, taken in
                                    * the order they appear) */
    int32_t paired;                /* ORD: two files (!singleReadsMode), rows [T/2 * p, T/2 * (p+1)) */
    int32_t rev_compl_pair_file;   /* PE / ORD: applyRevComplPairFileToPgs (pgrc-decoder.cpp:700-724) -- the HQ RC flag of
                                    * the rows of file 2 (PE: odd i; ORD: i >= T/2) is flipped */
} pgrc_decode_order;
/* The order of the following pgrc_decode_rows calls: uploads it, checks it (PGRC_E_PARAM on an index out of range or a
 * window past the text end) and makes the ORD ranks.  Needs every list added. */
int pgrc_decode_set_order(pgrc_decode_ctx *ctx, const pgrc_decode_order *order);
/* files of the order (SE 1, PE 2, ORD 1 or 2) and rows of one of them */
int pgrc_decode_row_count(pgrc_decode_ctx *ctx, uint32_t file, uint64_t *n_rows);
/* rows [first, first+n) of output file `file` into out: n * (L+1) bytes, each row L symbols + '\n'.  A caller streams a
 * large output in pieces; pinned (page-locked) host memory is written by the device directly, other memory through the
 * context's pinned staging buffers. */
int pgrc_decode_rows(pgrc_decode_ctx *ctx, uint32_t file, uint64_t first, uint64_t n, char *out);
/* the same into device memory (16-byte aligned) on the context's stream, without a copy down (tools, chained work) */
int pgrc_decode_rows_device(pgrc_decode_ctx *ctx, uint32_t file, uint64_t first, uint64_t n, void *d_out);

/* device time (HIP events) and host wall time of the context's last calls */
typedef struct {
    float ms_text;              /* set_text: host wall time of the upload */
    float ms_lists_device;      /* add_list: device time of the scans and checks, summed since set_text */
    float ms_order_device;      /* set_order: device time of its checks and the ORD rank scan */
    float ms_rows_device;       /* last rows / rows_device: device time of the row kernels */
    float ms_rows;              /* last rows / rows_device: host wall time of the call */
    uint64_t rows_bytes;        /* last rows / rows_device: bytes written */
} pgrc_decode_timing;
int pgrc_decode_get_timing(pgrc_decode_ctx *ctx, pgrc_decode_timing *out);

/* ---- The matched pseudogenomes (the inverse of row f2, SimplePgMatcher::restoreMatchedPgs, SimplePgMatcher.cpp:259-351).
 * The encoder's markAndRemoveExactMatches replaced every matched stretch of each pseudogenome by one '%' and wrote, per
 * mark, a source offset into the ORIGINAL HQ text (4 bytes little-endian when org_hq_len <= UINT32_MAX, else 8) and a
 * length (byte-frugal: 7 bits per byte, low group first, high bit = more bytes; the stream starts with minMatchLength
 * and every mark's value is its length minus it).  A mark's text is the reverse complement (complementsLut) of
 * src[off, off+len) -- the plain substring when rev_compl is 0.  HQ restores from itself (a mark may copy what an
 * earlier mark produced), LQ and N from the restored HQ. */
typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_decode_mapped) */
    const char *mapped;             /* comboPgMapped: the mapped HQ, LQ and N one after the other */
    uint64_t mapped_len[3];         /* hqPgMappedLen, lqPgMappedLen, nPgMappedLen (0 with empty streams: no such part) */
    uint64_t org_hq_len;            /* orgHqPgLen: the restored HQ length; also decides the offset width of all parts */
    const uint8_t *map_off[3];      /* per part: the offsets stream */
    uint64_t map_off_bytes[3];
    const uint8_t *map_len[3];      /* per part: the byte-frugal lengths stream (empty: no marks, minMatchLength 0) */
    uint64_t map_len_bytes[3];
    int32_t rev_compl;              /* revComplMatching: 1 in every call of the reference's decoder */
} pgrc_decode_mapped;
/* Restores the three parts on the device and installs the joined restored text HQ | LQ | N, as pgrc_decode_set_text
 * would with that text (the lists and the order are dropped).  PGRC_E_PARAM, with no text installed afterwards, when the
 * marks and the stream values disagree in number, a byte-frugal value is longer than 10 bytes or runs past its stream's
 * end, an offsets stream is not marks x width bytes, a source range reaches past the HQ end, an HQ mark's source reaches
 * its own output position, or the restored HQ length differs from org_hq_len. */
int pgrc_decode_set_mapped_text(pgrc_decode_ctx *ctx, const pgrc_decode_mapped *m);
/* The same with the joined mapped text still in the form the archive holds it in: the payload of
 * VarLenDNACoder::Compress (pgrc_varlen.h), which restoreMatchedPgs gets from VarLenDNACoder::Uncompress.  m->mapped must be
 * NULL; the sum of m->mapped_len[] is the expected decoded length.  The coded bytes go up (about 0.3 byte a symbol), `v`
 * decodes them in HBM and the restore runs unchanged.  PGRC_E_PARAM: a decoded length that differs from the expected one
 * (the reference exits there), a coder on another device, v or (with coded_len > 0) coded NULL.  Every failure leaves no
 * text installed.  pgrc_varlen_timing(v) reports the decode; pgrc_decode_get_restore_timing counts it in ms_upload. */
int pgrc_decode_set_mapped_text_coded(pgrc_decode_ctx *ctx, const pgrc_decode_mapped *m, pgrc_varlen *v, const void *coded,
                                      uint64_t coded_len);
/* the restored HQ, LQ and N lengths (the lists' text_base: 0, lens[0], lens[0] + lens[1]); PGRC_E_STATE unless the text
 * came from pgrc_decode_set_mapped_text */
int pgrc_decode_text_lengths(pgrc_decode_ctx *ctx, uint64_t lens[3]);
/* bytes [first, first+n) of the installed joined text into out (pinned memory directly, other memory in chunks through
 * the context's staging buffers) */
int pgrc_decode_get_text(pgrc_decode_ctx *ctx, uint64_t first, uint64_t n, char *out);

typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_decode_restore_timing) */
    float ms_upload;                /* host wall time of the upload of the mapped text and the streams */
    float ms_parse_device;          /* device time: marks, stream values, offsets, output positions, checks */
    float ms_literals_device;       /* device time: the literal runs shifted to their output positions */
    float ms_matches_device;        /* device time: HQ chain resolution and the fill of every part's matches */
    float ms_call;                  /* host wall time of the whole call */
    uint32_t passes;                /* pointer-jumping passes of the HQ chain resolution */
    uint64_t marks[3];              /* marks per part */
    uint64_t matched[3];            /* matched (restored from a source) symbols per part */
} pgrc_decode_restore_timing;
/* of the last successful pgrc_decode_set_mapped_text */
int pgrc_decode_get_restore_timing(pgrc_decode_ctx *ctx, pgrc_decode_restore_timing *out);

/* ---- The pair-position coding of the order-preserving paired mode (SeparatedPseudoGenomePersistence::
 * compressReadsPgPositions, SeparatedPseudoGenomePersistence.cpp:445-574, and decompressReadsPgPositions, :582-673; not
 * singleFileMode, delta coding on, i.e. archives of version >= 1.3).  T = readsTotalCount (even) reads are P = T/2 pairs;
 * positions are W = pos_width bytes wide (4 iff the joined Pg length <= UINT32_MAX, pgrc-decoder.cpp:805).
 *
 * The base read's position of every pair goes out as it is, in PAIR order.  The pairs are then ranked by base position
 * (stable: ties by pair number) and every mate is coded in RANK order, with rel = |mate - base| in W bytes:
 *   near   rel <= 65535: off16_flag 1, a base-first flag (base < mate, strictly) and rel as uint16
 *   far    otherwise: off16_flag 0 and a delta16_flag --
 *     delta  rel - refPrev fits int16: delta16_flag 1, a base-first flag, the difference; refPrev = rel
 *     full   otherwise: delta16_flag 0 and the mate's position itself; refPrev = rel, unless the far pair before this one
 *            was a delta pair: then refPrev stays (:521)
 * refPrev starts as 0.  The three scalars of the reference's serial loop are a three-state machine over the far pairs (the
 * pair before was a delta pair / a full pair that kept refPrev / a full pair that set it): the encoder finds
 * every pair's state with one scan of state maps, the decoder refPrev with one segmented sum, and everything else is
 * prefix scans of the flags, all on the device; the rank order is radix.hip's stable sort.
 *
 * All three calls work on a decode context (its stream, staging buffers and error string) and need no text.  P is limited
 * to the radix sort's record count (below 0xFFFFF000 pairs). */
typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_pairpos_streams) */
    uint32_t pos_width;             /* W: 4 or 8 */
    uint64_t n_total;               /* T: readsTotalCount, even */
    const void *base_pos;           /* basePairPos: T/2 positions of W bytes, pair order */
    const uint8_t *off16_flag;      /* offsetInUint16Flag: T/2 flags, rank order (1 = near) */
    const uint8_t *off_base_first;  /* offsetIsBaseFirstFlag: n_off16 */
    const uint16_t *off_value;      /* offsetInUint16Value: n_off16 */
    const uint8_t *delta16_flag;    /* deltaInInt16Flag: n_delta_flag, one per far pair (non-zero = delta) */
    const uint8_t *delta_base_first;/* deltaIsBaseFirstFlag: n_delta16 */
    const int16_t *delta_value;     /* deltaInInt16Value: n_delta16 */
    const void *not_base_pos;       /* notBasePairPos: n_not_base positions of W bytes */
    uint64_t n_off16, n_delta_flag, n_delta16, n_not_base;     /* elements of the variable-length streams (off_base_first
                                                                * and off_value share n_off16, delta_base_first and
                                                                * delta_value n_delta16) */
} pgrc_pairpos_streams;

/* compressReadsPgPositions: org_idx_to_pos holds T positions with the mates INTERLEAVED ([2p] = the base read of pair p,
 * [2p+1] its mate), as the reference's encoder has them.  On success *out describes the eight streams in ONE block of
 * page-locked host memory that the library allocated (it starts at out->base_pos) and pgrc_pairpos_free gives back.
 * PGRC_E_PARAM: odd n_total, pos_width not 4 or 8, a position >= 2^32 with pos_width 4, too many pairs. */
int pgrc_pairpos_encode(pgrc_decode_ctx *ctx, const uint64_t *org_idx_to_pos, uint64_t n_total, uint32_t pos_width,
                        pgrc_pairpos_streams *out);
void pgrc_pairpos_free(pgrc_pairpos_streams *streams);   /* of pgrc_pairpos_encode only; clears the struct */

/* decompressReadsPgPositions: the positions as T uint64, FILE-MAJOR ([p] = the base read of pair p, [T/2 + p] its mate --
 * the layout of pgrc_decode_order.org_idx_to_pos with paired = 1), each truncated to W bytes as the reference's store
 * does.  PGRC_E_PARAM (the reference reads past its vectors in these cases): odd n_total, pos_width not 4 or 8, a NULL
 * stream with a non-zero count, ones in off16_flag != n_off16, its other flags != n_delta_flag, non-zero flags in
 * delta16_flag != n_delta16, its zeros != n_not_base, too many pairs. */
int pgrc_pairpos_decode(pgrc_decode_ctx *ctx, const pgrc_pairpos_streams *streams, uint64_t *pg_pos);

/* What pgrc_decode_set_order does for mode = PGRC_DECODE_ORD, paired = 1, with the positions decoded on the device
 * straight into the context's order: the array never exists on the host.  Every check of pgrc_decode_set_order runs on
 * the decoded positions; after any failure the context has no order. */
int pgrc_decode_set_order_pair_streams(pgrc_decode_ctx *ctx, const pgrc_pairpos_streams *streams, int32_t rev_compl_pair_file);
/* What pgrc_decode_set_order does for mode = PGRC_DECODE_ORD, paired = 0, from the array as the single-file archive holds it
 * (decompressReadsPgPositions with singleFileMode): n_total positions of pos_width (4 or 8) bytes each, uploaded as they are
 * and widened on the device into the context's order.  Every check of pgrc_decode_set_order runs on the widened positions;
 * after any failure the context has no order.  PGRC_E_PARAM: a width other than 4 or 8, NULL with n_total > 0. */
int pgrc_decode_set_order_positions(pgrc_decode_ctx *ctx, const void *positions, uint32_t pos_width, uint64_t n_total,
                                    int32_t rev_compl_pair_file);

typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_pairpos_timing) */
    int32_t encode;                 /* 1 = the last call was pgrc_pairpos_encode, 0 = a decode */
    float ms_upload;                /* host wall time until the input was queued for the device */
    float ms_sort_device;           /* device time: records and the rank order (radix sort) */
    float ms_scan_device;           /* device time: classification, the flag scans and (encode) the chain */
    float ms_scatter_device;        /* device time: compaction of the streams (encode) / the chain's scan, whose last pass scatters the mates (decode) */
    float ms_download;              /* host wall time of the copy down (encode, pgrc_pairpos_decode) */
    float ms_call;                  /* host wall time of the whole call (of set_order_pair_streams: its checks included) */
    uint64_t bytes_up, bytes_down;
    uint64_t n_near, n_delta, n_full;   /* pairs by kind */
} pgrc_pairpos_timing;
/* of the context's last successful pair-position call */
int pgrc_pairpos_get_timing(pgrc_decode_ctx *ctx, pgrc_pairpos_timing *out);

/* ---- The pair-order coding of the paired mode that does NOT preserve the order (SeparatedPseudoGenomePersistence::
 * compressReadsOrder, SeparatedPseudoGenomePersistence.cpp:220-339, called from pgrc-encoder.cpp:223) and its decoder
 * (decompressReadsOrder, :341-443).  The decoder is a true recurrence -- the k-th pair lands on the k-th entry that no
 * earlier pair has marked -- so its landing is ONE wave's sweep over the entries, 64 at a time, with everything around it
 * (the offsets of all pairs, the forms' tails, the checks) parallel: pgrc_pairorder_decode.h, included at the end of this
 * header.
 *
 * T = readsCount (even, below 2^32) entries of the joined reads lists HQ | LQ | N; org[i] is entry i's original index, a
 * permutation of [0, T); reads 2q and 2q+1 are mates.  With rev[org[i]] = i the mate of entry i is rev[org[i] ^ 1].
 * Entry i is a BASE iff its mate lies after it; the P = T/2 bases, in entry order, number the pairs.  Pair k with base i
 * and rel = mate - i >= 1 is
 *   near   rel <= 255: off8_flag[k] 1 and rel as uint8
 *   far    otherwise: off8_flag[k] 0 and a delta8_flag --
 *     delta  rel - refPrev fits int8: delta8_flag 1 and the difference; refPrev = rel
 *     full   otherwise: delta8_flag 0 and rel as uint32; refPrev = rel, unless the far pair before this one was a delta
 *            pair: then refPrev stays (:290)
 * refPrev starts as 0: the chain of the pair-position coding above with int8 for int16, run by the same kernels.
 *
 * The forms are the combinations of the reference's (completeOrderInfo, ignorePairOrderInformation, singleFileMode) that
 * write different streams ("*" = either value): */
enum {
    PGRC_PAIRORDER_IGNORE = 0,              /* (false, true, *): the five common streams -- off8_flag, off_value, delta8_flag,
                                             * delta_value, full_offset -- and nothing else */
    PGRC_PAIRORDER_FILE_FLAGS = 1,          /* (false, false, *): the five, and the base's file (org[i] & 1) per pair in
                                             * off_base_file_flag (near pairs) and nonoff_base_file_flag (far pairs) */
    PGRC_PAIRORDER_COMPLETE = 2,            /* (true, *, false): the five, and pair_base_org_idx[org[i] / 2] = 2k + (org[i] & 1)
                                             * for the base i of every pair k (revPairBaseOrgIdx) */
    PGRC_PAIRORDER_COMPLETE_SINGLE_FILE = 3 /* (true, *, true): rev alone, T uint32 */
};

typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_pairorder_streams) */
    int32_t form;                   /* PGRC_PAIRORDER_* */
    uint64_t n_total;               /* T: readsCount, even */
    const uint8_t *off8_flag;       /* offsetInUint8Flag: T/2 flags, pair order (1 = near); the START OF THE BLOCK in every
                                     * form, also where it holds no element */
    const uint8_t *off_value;       /* offsetInUint8Value: n_off8 */
    const uint8_t *delta8_flag;     /* deltaInInt8Flag: n_delta_flag, one per far pair */
    const int8_t *delta_value;      /* deltaInInt8Value: n_delta8 */
    const uint32_t *full_offset;    /* fullOffset: n_full */
    const uint32_t *pair_base_org_idx;      /* revPairBaseOrgIdx: T/2 (COMPLETE; NULL otherwise) */
    const uint8_t *off_base_file_flag;      /* offsetPairBaseFileFlag: n_off8 (FILE_FLAGS; NULL otherwise) */
    const uint8_t *nonoff_base_file_flag;   /* nonOffsetPairBaseFileFlag: n_delta_flag (FILE_FLAGS; NULL otherwise) */
    const uint32_t *rev;            /* T (COMPLETE_SINGLE_FILE; NULL otherwise) */
    uint64_t n_off8, n_delta_flag, n_delta8, n_full;    /* elements of the variable-length streams (all 0 with
                                                         * COMPLETE_SINGLE_FILE, where off8_flag holds no element either) */
} pgrc_pairorder_streams;

/* compressReadsOrder: org_idx[l] holds the n[l] original indexes of list l (HQ, LQ, N) as the lists have them; the joined
 * array is never made on the host (NULL with n[l] = 0: no such list).  On success *out describes the streams in ONE block
 * of page-locked host memory that the library allocated (it starts at out->off8_flag) and pgrc_pairorder_free gives back.
 * PGRC_E_PARAM, where the reference's behaviour is undefined: a total that is odd or 2^32 or more, a value >= T, a
 * value that occurs twice, an unknown form, a NULL list with a non-zero count.  After any failure *out is cleared and the
 * context stays usable.  Works on a decode context (its stream, staging buffers and error string) and needs no text. */
int pgrc_pairorder_encode(pgrc_decode_ctx *ctx, const uint32_t *const org_idx[3], const uint64_t n[3], int32_t form,
                          pgrc_pairorder_streams *out);
void pgrc_pairorder_free(pgrc_pairorder_streams *streams);   /* of pgrc_pairorder_encode; clears the struct */

typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_pairorder_timing) */
    int32_t form;
    float ms_upload;                /* host wall time until the input was queued for the device */
    float ms_inverse_device;        /* device time: the scatter of rev and the classification (mate, base flag, rel) */
    float ms_scatter_device;        /* ... of which the scatter alone (with the sentinel fill queued before it) */
    float ms_scan_device;           /* device time: the three flag scans and the chain (maps, map scan, kinds) */
    float ms_compact_device;        /* device time: pair order, pair_base_org_idx, the near, far, delta and full streams */
    float ms_download;              /* host wall time: the page-locked block and the copy down */
    float ms_call;                  /* host wall time of the whole call */
    uint64_t bytes_up, bytes_down;
    uint64_t n_near, n_delta, n_full;   /* pairs by kind (0 with COMPLETE_SINGLE_FILE: no pair is coded) */
} pgrc_pairorder_timing;
/* of the context's last successful pgrc_pairorder_encode */
int pgrc_pairorder_get_timing(pgrc_decode_ctx *ctx, pgrc_pairorder_timing *out);

/* The decoder of this coding -- decompressReadsOrder on the device and the PE order straight from the streams -- is declared
 * in pgrc_pairorder_decode.h, which this header includes at its end. */

/* ---- The archive form of a reads list's mismatch streams (SeparatedPseudoGenomeOutputBuilder::compressedBuild,
 * SeparatedPseudoGenomePersistence.cpp:905-952, and the loader's inverse, ExtendedReadsListWithConstantAccessOption::
 * loadConstantAccessExtendedReadsList, SeparatedExtendedReadsList.cpp:210-294).  The builder's
 * writeReadEntry appends one count per entry, one context code (actual << 4) + mismatch per mismatch and one rev-coded
 * offset per mismatch (pgrc_export_streams); the archive holds them reshaped:
 *   zero flags   toStringAndSeparateZeros (:801-813): zero_flags[i] = (mis_cnt[i] == 0), and the non-zero counts in entry
 *                order
 *   symbols      reorderingSymbolsExclusiveMismatchEncoding (:1115-1138): the mismatch VALUES (low nibbles) are counted,
 *                the five values ordered by descending count (ties keep A C G T N), bases_order = the symbols in that order,
 *                and every code becomes rev[mismatch] - (rev[mismatch] > rev[actual]), rev = the place of a value in it
 *   offsets      compressRlMisRevOffDest (:823-903): an entry with count c sends its c bytes, in stream order, to
 *                destination c (1 <= c <= 254).  limit = the largest non-empty destination (0 without mismatches); the
 *                props bytes are [limit, 1, 2, ..., limit - 1].  With CODER_LEVEL_FAST the props are [1] and destination 1
 *                is the unsplit stream.  (separateFirstOffsetMode and transposeMode are off in every call of the reference.)
 * All of it is flags, prefix sums, a five-bin histogram and ONE stable split of the entries by their count: a count matrix
 * (count, tile) over tiles of PGRC_LIST_ARCHIVE_TILE entries, its scan, and ballot ranks inside a tile.  No merged stream is
 * made on the host in either direction.
 *
 * Limits: offsets of ONE byte (the loader reads them into vector<uint8_t>), n_entries < 2^32 and n_mismatches < 2^32
 * (PGRC_E_PARAM otherwise).  The calls work on a decode context (its stream, staging buffers and error string). */
#define PGRC_LIST_ARCHIVE_TILE 8192u    /* entries of one tile of the split */
typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_list_archive_streams) */
    uint32_t props_len;             /* bytes of props: max(1, limit) */
    uint64_t n_entries, n_mismatches, n_nonzero;
    const uint8_t *zero_flags;      /* n_entries; the START OF THE BLOCK of pgrc_list_archive_encode */
    const uint8_t *nonzero_cnt;     /* n_nonzero */
    const uint8_t *mis_sym;         /* n_mismatches exclusive codes (0 .. 3; 4 only where actual == mismatch == the last value) */
    char bases_order[5];            /* the five symbols by descending count of their value */
    uint32_t n_dests;               /* limit: props[0] */
    const uint8_t *props;           /* [limit, 1, ..., limit - 1], or [0] */
    const uint8_t *dest[255];       /* index 1 .. n_dests: the offsets of the entries with that count; [0] unused */
    uint64_t dest_len[255];         /* bytes of dest[c]: c * (entries with count c); n_mismatches for the one stream of [1] */
    void *block;                    /* encode: the one page-locked block all streams lie in (= zero_flags) */
} pgrc_list_archive_streams;

/* compressedBuild's reshaping of in->mis_cnt, in->mis_sym and in->mis_rev_off (in->off_width must be 1).  fast_level != 0:
 * CODER_LEVEL_FAST.  On success *out describes the streams in ONE block of page-locked host memory that the library
 * allocated, filled by one copy from the device; the destinations lie one behind the other in it; pgrc_list_archive_free
 * gives it back.  PGRC_E_PARAM: off_width != 1, 2^32 entries or mismatches or more, a NULL stream with a non-zero count,
 * n_mismatches != the sum of the counts, a nibble of a code above 4, a count of 255 at the normal level (it indexes past
 * the reference's 255-element map).  After any failure *out is cleared and the context stays usable. */
int pgrc_list_archive_encode(pgrc_decode_ctx *ctx, const pgrc_export_streams *in, int32_t fast_level, pgrc_list_archive_streams *out);
void pgrc_list_archive_free(pgrc_list_archive_streams *streams);   /* of pgrc_list_archive_encode; clears the struct */

/* pgrc_decode_add_list with the list's mismatches still in the archive's form: `list` carries text_base, n_entries, off /
 * pos and rev_comp as for pgrc_decode_add_list and its mis_* pointers must be NULL; `s` goes up as it is, the per-entry
 * tables are rebuilt on the device (counts from the flags, every entry's offsets gathered from the source of its count at
 * c * (entries before it with count c) and turned into forward offsets on the way) and the context is left as
 * pgrc_decode_add_list leaves it with the reassembled streams (mis_sym_form 0, rev-coded offsets, s->bases_order).
 * With limit = 1 every entry takes its bytes from the one stream at its mismatch-list start, whatever its count (the
 * loader maps every count to the last source).  Refused with PGRC_E_PARAM before any table is kept: entries without a zero
 * flag != n_nonzero, a count above limit (limit != 1), props other than the ones the reference writes (limit <= 254,
 * props[m] == m), dest_len[c] != c * (entries with count c), n_mismatches != the sum of the counts, n_entries !=
 * list->n_entries, and everything pgrc_decode_add_list refuses. */
int pgrc_decode_add_list_archive(pgrc_decode_ctx *ctx, const pgrc_decode_list *list, const pgrc_list_archive_streams *s);

typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_list_archive_timing) */
    int32_t encode;                 /* 1 = the last call was pgrc_list_archive_encode, 0 = pgrc_decode_add_list_archive */
    float ms_upload;                /* host wall time until the streams were queued for the device */
    float ms_flags_device;          /* device time: the flag scan, zero flags / counts, the mismatch-list starts */
    float ms_symbols_device;        /* device time: histogram and recode (encode) / the check of the codes (decode) */
    float ms_split_device;          /* device time: count matrix, its scan, scatter (encode) / gather with the conversion (decode) */
    float ms_download;              /* host wall time: the page-locked block and the copy down (encode) */
    float ms_call;                  /* host wall time of the whole call (decode: positions and RC flags of the list included) */
    uint64_t bytes_up, bytes_down;
    uint64_t n_nonzero, limit;
} pgrc_list_archive_timing;
/* of the context's last successful pgrc_list_archive_encode or pgrc_decode_add_list_archive */
int pgrc_list_archive_get_timing(pgrc_decode_ctx *ctx, pgrc_list_archive_timing *out);

#include "pgrc_pairorder_decode.h"

#ifdef __cplusplus
}
#endif
#endif /* PGRC_DECODE_H */
