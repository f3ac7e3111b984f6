/*
 * pgrc_assemble.h -- C ABI of libpgrc_match.so, part 5: the assembly of a pseudogenome from the overlap graph on MI355X.
 *
 * Drop-in boundary: what AbstractOverlapPseudoGenomeGeneratorTemplate does once findOverlappingReads has filled
 * nextRead[] and overlap[] (pseudogenome/generator/AbstractOverlapPseudoGenomeGenerator.cpp):
 *   removeCyclesAndPrepareComponents  (:6-41)     every cycle is cut at its LARGEST read index m: nextRead[m] = 0,
 *                                                 overlap[m] = 0 (the two locals shadowed at :20-21 keep the cut at the read
 *                                                 that closes the cycle, and the loop meets a cycle at its largest index)
 *   countPseudoGenomeLength           (:146-153)  pgLen = sum of read_len - overlap[i]
 *   assemblePseudoGenomeTemplate      (:183-219)  the heads (reads without a predecessor, singles included) in ascending
 *                                                 index, each chain to its end: entry j of the reads list gets the read's
 *                                                 original index and off[j] = read_len - overlap[read of entry j - 1]
 *                                                 (off[0] = 0; across chain ends the overlap is 0), and the text is the
 *                                                 reads laid over one another at those offsets
 *   applyIndexesMapping                           orgIdx[j] = mapping[orgIdx[j]]
 * Reads are numbered 1 .. R as the reference does (incIdx; 0 = no successor); read i is row i - 1 of a
 * PackedConstantLengthReadsSet in the layouts include/pgrc_reads.h describes.
 *
 * The parallel form writes every text byte once: entry j contributes its first read_len - overlap symbols.
 * That equals the reference's text exactly when every link's overlap is real -- the last overlap[i] symbols of read i are
 * the first overlap[i] symbols of nextRead[i] -- so every link is verified on the device (a cut link too, before the cut)
 * and an input with a false overlap is refused.
 *
 * Same conventions as pgrc_match.h: 0 = success, PGRC_E_* otherwise; host buffers stay the caller's; no CPU fallback --
 * without a HIP device pgrc_asm_create fails with PGRC_E_NO_DEVICE.
 */
#ifndef PGRC_ASSEMBLE_H
#define PGRC_ASSEMBLE_H

#include <stddef.h>
#include <stdint.h>

#include "pgrc_match.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgrc_asm_ctx pgrc_asm_ctx;

int pgrc_asm_create(int32_t device, pgrc_asm_ctx **out);      /* device: HIP device, -1 = the current one */
void pgrc_asm_destroy(pgrc_asm_ctx *ctx);
const char *pgrc_asm_last_error(const pgrc_asm_ctx *ctx);     /* NULL: the last failed create of this thread */

typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_asm_input) */
    uint32_t read_len;              /* L: 1 .. 255 */
    uint32_t symbols;               /* 4 = "ACGT" (4 symbols per byte), 5 = "ACGNT" (3 per byte) */
    uint32_t overlap_width;         /* bytes of an element of `overlap`: 1 (uint_read_len_min) or 2 (uint_read_len_std) */
    uint64_t n_reads;               /* R: 1 .. 2^32 - 2 */
    const uint8_t *packed_rows;     /* packedReads: R rows of (L + 3) / 4 or (L + 2) / 3 bytes */
    const uint32_t *next_read;      /* nextRead[0 .. R]; element 0 is ignored */
    const void *overlap;            /* overlap[0 .. R] in overlap_width bytes; element 0 is ignored */
    const uint32_t *index_mapping;  /* R original indexes (applyIndexesMapping), or NULL: orgIdx = read index - 1 */
} pgrc_asm_input;

typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_asm_result) */
    uint32_t reserved;
    uint64_t pg_len;                /* pseudoGenomeLength after the cuts */
    uint64_t n_reads;               /* R: entries of the two arrays */
    uint64_t cycles;                /* "Removed <cycles> cycles (lost <overlap_lost> symbols)"; the sum is kept in 64 bits
                                     * (the reference adds it up in uint_reads_cnt) */
    uint64_t overlap_lost;
    uint64_t components;            /* heads with a successor, after the cuts (countComponents) */
    uint64_t singles;               /* heads without one (countSingles) */
    const uint32_t *org_idx;        /* R: the reads list's original indexes, walk order; the START OF THE BLOCK */
    const uint16_t *off;            /* R: the reads list's offsets */
} pgrc_asm_result;

/* The whole of part 2.  On success *out describes the reads list in ONE block of page-locked host memory that the library
 * allocated (it starts at out->org_idx) and pgrc_asm_free_result gives back; the text stays on the device (below).
 * PGRC_E_PARAM, with *out cleared, no text installed and the context still usable: a NULL pointer, a wrong struct_size,
 * read_len, symbols, overlap_width or n_reads out of range; next_read[i] > R; a read with two predecessors;
 * overlap[i] > L; overlap[i] != 0 where next_read[i] == 0; a link whose overlap is not real; a row byte that is no
 * packing (5 symbols: a byte >= 125, or a non-zero digit after symbol L - 1). */
int pgrc_asm_run(pgrc_asm_ctx *ctx, const pgrc_asm_input *in, pgrc_asm_result *out);
void pgrc_asm_free_result(pgrc_asm_result *res);    /* of pgrc_asm_run; clears the struct */

/* n bytes of the ASCII text from `first` on.  Page-locked memory is written directly, other memory through the context's
 * staging buffers.  PGRC_E_STATE before a successful run, PGRC_E_PARAM beyond pg_len. */
int pgrc_asm_get_text(pgrc_asm_ctx *ctx, uint64_t first, uint64_t n, char *out);

/* The text where the last run left it: pg_len bytes of ASCII on the context's device. */
int pgrc_asm_text_device(pgrc_asm_ctx *ctx, const void **d_ascii, uint64_t *len);
/* The same at 2 bits per symbol, the layout pgrc_match_set_pg_packed_device takes ((pg_len + 15) / 16 words); made on the
 * first request after a run.  symbols == 4 only (PGRC_E_PARAM otherwise).
 * Both device pointers are valid until the context's next run or its destruction. */
int pgrc_asm_packed_device(pgrc_asm_ctx *ctx, const void **d_words);

typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_asm_timing) */
    uint32_t passes_cycles;         /* pointer-jumping passes of the cycle search / of the ranking */
    uint32_t passes_rank;
    float ms_upload;                /* host wall time until the input was queued for the device */
    float ms_checks_device;         /* device time: the inverse (pred), the range checks, the links verified, the rows checked */
    float ms_cycles_device;         /* device time: jumping on next with the running maximum, the cuts */
    float ms_rank_device;           /* device time: jumping on pred with (head, distance) */
    float ms_lists_device;          /* device time: chain lengths, their scan, the walk order, off, orgIdx, the scan of the shifts */
    float ms_text_device;           /* device time: the text tiles */
    float ms_download;              /* host wall time: the page-locked block and the copy down */
    float ms_call;                  /* host wall time of the whole call */
    uint64_t bytes_up, bytes_down;
} pgrc_asm_timing;
/* of the context's last successful pgrc_asm_run */
int pgrc_asm_get_timing(pgrc_asm_ctx *ctx, pgrc_asm_timing *out);

#ifdef __cplusplus
}
#endif
#endif /* PGRC_ASSEMBLE_H */
