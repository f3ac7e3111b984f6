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
 * Here the host hands over the joined text and the reassembled per-entry streams of every list (entropy decoding and
 * archive parsing stay with the caller); positions and mismatch list starts are prefix scans on the device, every row
 * is an independent job of a row kernel that assembles tiles of rows in LDS, and rows come back to the host in chunks
 * copied down while the next chunk is made.
 *
 * Same conventions as pgrc_match.h: 0 = success, PGRC_E_* otherwise; host buffers stay the caller's (nothing is
 * borrowed beyond a call); no CPU fallback -- without a HIP device every call fails.
 */
#ifndef PGRC_DECODE_H
#define PGRC_DECODE_H

#include <stddef.h>
#include <stdint.h>

#include "pgrc_match.h"

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

#ifdef __cplusplus
}
#endif
#endif /* PGRC_DECODE_H */
