/*
 * pgrc_overlap.h -- C ABI of libpgrc_match.so, part 6: the overlap search of the pseudogenome generator on MI355X.
 *
 * Drop-in boundary: findOverlappingReads of GreedySwipingPackedOverlapGeneratorTemplate, the generator the encoder uses at
 * one thread (pseudogenome/generator/GreedySwipingPackedOverlapPseudoGenomeGenerator.cpp):
 *   initAndFindDuplicates<false>                    (:97-136)   the reads in sorted order; a run of equal reads d1 .. dk becomes a
 *                                                               chain nextRead[d_t] = d_(t+1), overlap[d_t] = L
 *   overlapSortedReadsAndMergeSortSuffixes<false>   (:171-249)  sweep i = 1 .. iters - 1, iters = (uint_read_len)(L * stop_coef):
 *                                                               the suffixes from symbol i on of the reads without a successor
 *                                                               are merged with the prefixes of L - i symbols of the reads
 *                                                               without a predecessor; equal ones are linked with overlap L - i
 * and getBothSidesOverlappedReads of AbstractOverlapPseudoGenomeGeneratorTemplate (AbstractOverlapPseudoGenomeGenerator.cpp:75-91).
 * Reads are numbered 1 .. R as the reference does (0 = none); read i is row i - 1 of a PackedConstantLengthReadsSet in the
 * layouts include/pgrc_reads.h describes.  Strings compare as compareSequences does: by symbol in the alphabet's order.
 *
 * The reference's sweep is one loop over a queue of groups; the device runs the same decisions as ranks inside runs of equal
 * suffixes, a weak order of the five groups folded over the runs with an associative operator, a search per run in the prefix
 * list and a closed form of the pairing.  nextRead, overlap and the reads-left numbers of the reference's log
 * are reproduced exactly, GIVEN THE ORDER AMONG EQUAL READS: the reference sorts with an unstable sort, so which of two equal
 * reads comes first there is unspecified, and it decides which of them ends a chain of duplicates and takes part in the sweeps.
 * A caller that must reproduce one particular run of the reference passes that run's sorted order (`sorted_order`); with NULL
 * the order is made on the device by a stable sort of the rows, equal reads in ascending number -- a valid outcome of the
 * reference's sort, which differs from any other only in the order inside runs of equal reads.
 *
 * The encoder takes ParallelGreedySwipingPackedOverlapGeneratorTemplate instead when it runs with more than one thread on a set of
 * more than 50 000 reads; its findOverlappingReads is reproduced under PGRC_OVL_RULE_PARALLEL (pgrc_ovl_set_rule below,
 * DESIGN.md 4.18).  avoidCyclesMode is not covered.
 *
 * Same conventions as pgrc_assemble.h: 0 = success, PGRC_E_* otherwise; struct sizes are checked; host buffers stay the
 * caller's; no CPU fallback -- without a HIP device pgrc_ovl_create fails with PGRC_E_NO_DEVICE.
 */
#ifndef PGRC_OVERLAP_H
#define PGRC_OVERLAP_H

#include <stddef.h>
#include <stdint.h>

#include "pgrc_assemble.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgrc_ovl_ctx pgrc_ovl_ctx;

int pgrc_ovl_create(int32_t device, pgrc_ovl_ctx **out);      /* device: HIP device, -1 = the current one */
void pgrc_ovl_destroy(pgrc_ovl_ctx *ctx);
const char *pgrc_ovl_last_error(const pgrc_ovl_ctx *ctx);     /* NULL: the last failed create of this thread */

typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_ovl_input) */
    uint32_t read_len;              /* L: 1 .. 255 */
    uint32_t symbols;               /* 4 = "ACGT" (4 symbols per byte), 5 = "ACGNT" (3 per byte) */
    uint32_t overlap_width;         /* bytes of an element of the result's `overlap`: 1 (uint_read_len_min) or 2 */
    uint64_t n_reads;               /* R: 1 .. 2^32 - 2 */
    double stop_coef;               /* overlappedReadsCountStopCoef: 0 .. 1 */
    const uint8_t *packed_rows;     /* packedReads: R rows of (L + 3) / 4 or (L + 2) / 3 bytes */
    const uint32_t *sorted_order;   /* the read numbers 1 .. R in sorted order (sortedReadsIdxs after the sort of :105), or NULL:
                                     * made on the device, equal reads in ascending number */
} pgrc_ovl_input;

typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_ovl_result) */
    uint32_t sweeps;                /* iters - 1 (0 if iters < 2): the sweeps of the reference, run or known to change nothing */
    uint64_t n_reads;               /* R */
    uint64_t n_left;                /* entries of reads_left_after: max(iters, 1) */
    uint64_t duplicates;            /* "Found <duplicates> duplicates" (:135) */
    uint64_t links;                 /* links made by the sweeps */
    const uint32_t *next_read;      /* nextRead[0 .. R]; element 0 is 0; the START OF THE BLOCK */
    const void *overlap;            /* overlap[0 .. R] in overlap_width bytes */
    const uint64_t *reads_left_after; /* entry 0: readsLeft after the duplicates; entry i: "<n> reads left after <L - i> overlap" (:149) */
} pgrc_ovl_result;

/* The whole search.  On success *out describes ONE block of page-locked host memory that the library allocated (it starts at
 * out->next_read) and pgrc_ovl_free_result gives back; the rows, nextRead and overlap also stay on the device for
 * pgrc_ovl_both_sides and pgrc_ovl_assemble.
 * PGRC_E_PARAM, with *out cleared and the context still usable: a NULL pointer, a wrong struct_size, read_len, symbols,
 * overlap_width, n_reads or stop_coef out of range; a sorted_order that is no permutation of 1 .. R or in which a read is
 * followed by a smaller one (both checked on the device); a row byte that is no packing (5 symbols: a byte >= 125, or a
 * non-zero digit after symbol L - 1). */
int pgrc_ovl_run(pgrc_ovl_ctx *ctx, const pgrc_ovl_input *in, pgrc_ovl_result *out);
void pgrc_ovl_free_result(pgrc_ovl_result *res);    /* of pgrc_ovl_run; clears the struct */

/* getBothSidesOverlappedReads from the last run's nextRead and overlap: flags[i - 1] = 1 if read i has a predecessor and a
 * successor, or is linked to an equal read on either side; R bytes.  PGRC_E_STATE before a successful run. */
int pgrc_ovl_both_sides(pgrc_ovl_ctx *ctx, uint8_t *flags);

/* pgrc_asm_run on the last run's rows, nextRead and overlap, which go from this context to `asm_ctx` on the device (both
 * contexts on one device; no host round trip).  index_mapping: R original indexes or NULL.  Afterwards asm_ctx is as after a
 * pgrc_asm_run of its own (pgrc_asm_get_text, pgrc_asm_packed_device, pgrc_asm_free_result(asm_result), ...). */
int pgrc_ovl_assemble(pgrc_ovl_ctx *ctx, pgrc_asm_ctx *asm_ctx, const uint32_t *index_mapping, pgrc_asm_result *asm_result);

/* The rule of the sweeps.  PGRC_OVL_RULE_SERIAL (the default) is the generator of one thread.  PGRC_OVL_RULE_PARALLEL is
 * ParallelGreedySwipingPackedOverlapGeneratorTemplate::findOverlappingReads (ParallelGreedySwipingPackedOverlapPseudoGenomeGenerator.cpp;
 * avoidCyclesMode = false, where its threads only share out blocks and the result does not depend on their number):
 *   - a block is the set of strings with one prefix of three symbols; the order of the five groups in the merge starts anew, in
 *     symbol order, with every block, and a suffix that finds no prefix stays in the list (no drop rule);
 *   - the sweeps i >= L - 3 pair whole blocks of three, two and one symbols.  The suffixes of sweep L - 3 stand in the order
 *     of a merge whose compare runs past the reads' end into the packed rows behind them: by the reads x + 1, x + 2, ... that
 *     follow read x in the set, the groups popped smallest head first though they are not sorted by that key.  Behind the last
 *     row the reference reads memory that is not its own; here a missing row is below any row, and such compares are counted:
 *     the result is the reference's only if past_end_compares is 0.  The compares counted are the device's own: every suffix
 *     against the largest key before it in its group's share of the block, and the searches among the other groups' shares.
 *     Where no other read equals the last read of the set, only a compare with the last read can run past the end, and the
 *     device makes one whenever the reference does.  Where one does, two other reads whose followers agree up to the last
 *     row compare past the end as well, and the device's compares need not include that pair;
 *   - after the sweeps L - 3 and L - 2 what is left is regrouped by dropping the first symbol, in stable order.
 * read_len must be at least 4 under this rule (the reference reads symbol 3 of every read).
 * The two entry points are exported as pgrc_ovlrule_set and pgrc_ovlrule_get_info; pgrc_ovl_set_rule and
 * pgrc_ovl_get_rule_info are their names in this header. */
#define PGRC_OVL_RULE_SERIAL 0u
#define PGRC_OVL_RULE_PARALLEL 1u

typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_ovl_rule_info) */
    uint32_t rule;                  /* the rule of the run */
    uint32_t blocks;                /* symbols ^ 3 under the parallel rule, 0 under the serial one */
    uint32_t tail_sweeps;           /* 0 .. 3: the run's sweeps i >= L - 3, which pair whole blocks (0 under the serial rule) */
    uint64_t follower_compares;     /* compares decided by the rows that follow the two reads (the merge in front of sweep L - 3) */
    uint64_t past_end_compares;     /* ... of which ran past the last row */
} pgrc_ovl_rule_info;

/* Sets the rule of the context's later runs.  PGRC_E_PARAM: a NULL context or any other value.  Under the parallel rule
 * pgrc_ovl_run refuses read_len < 4 with PGRC_E_PARAM and leaves the context usable. */
int pgrc_ovlrule_set(pgrc_ovl_ctx *ctx, uint32_t rule);
/* of the context's last successful pgrc_ovl_run; PGRC_E_STATE before one */
int pgrc_ovlrule_get_info(pgrc_ovl_ctx *ctx, pgrc_ovl_rule_info *out);
#define pgrc_ovl_set_rule pgrc_ovlrule_set
#define pgrc_ovl_get_rule_info pgrc_ovlrule_get_info

typedef struct {
    uint32_t struct_size;           /* sizeof(pgrc_ovl_timing) */
    uint32_t passes;                /* sweeps that ran on the device (the rest had an empty list on one side) */
    float ms_upload;                /* host wall time until the input was queued for the device */
    float ms_order_device;          /* device time: the rows unpacked and checked, the order sorted or checked */
    float ms_start_device;          /* device time: the duplicates' chains, the two lists, the first groups */
    float ms_merge_device;          /* device time, all sweeps: ranks across the groups, the weak-order scan, the merged order */
    float ms_pair_device;           /* device time, all sweeps: every run's class in the prefix list, the pairing, the drop rule */
    float ms_compact_device;        /* device time, all sweeps: the two lists compacted, the next groups */
    float ms_download;              /* host wall time: the page-locked block and the copy down */
    float ms_call;                  /* host wall time of the whole call */
    uint64_t bytes_up, bytes_down;
} pgrc_ovl_timing;
/* of the context's last successful pgrc_ovl_run */
int pgrc_ovl_get_timing(pgrc_ovl_ctx *ctx, pgrc_ovl_timing *out);
/* device time of the sweeps 1 .. min(n, sweeps) of that run in ms (0 for a sweep that did not run) */
int pgrc_ovl_get_sweep_ms(pgrc_ovl_ctx *ctx, float *ms, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif /* PGRC_OVERLAP_H */
