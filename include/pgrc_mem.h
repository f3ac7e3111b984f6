/*
 * pgrc_mem.h -- C ABI of libpgrc_match.so, part 2: pseudogenome-vs-pseudogenome exact matching
 *  on MI355X.
 *
 * Drop-in boundary: the reference's TextMatcher seam (matching/TextMatchers.h:53-61).
 * SimplePgMatcher (matching/SimplePgMatcher.cpp:12-19) builds `new CopMEMMatcher(srcPg, len, targetMatchLength,
 * minMatchLength)` and calls `matcher->matchTexts(matches, destText, destIsSrc, revComplMatching, minMatchLength)`
 * (:24-55) once per destination pseudogenome.  The entry points below are what a `HipTextMatcher : TextMatcher`
 * binds (integration/HipTextMatcher.{h,cpp}); INTEGRATION.md shows the one-line change in SimplePgMatcher.
 *
 * Result semantics = CopMEMMatcher::matchTexts -> processExactMatchQueryTight
 * (matching/copmem/CopMEMMatcher.cpp:333-481, :604-622) over the SERIAL seed index (PgHelpers::numberOfThreads
 * == 1): the same matches in the same discovery order, including that scan's sequential skip rules and its
 * stale side-context registers near the text ends.
 *
 * Same conventions as pgrc_match.h: 0 = success, PGRC_E_* otherwise; host buffers stay the caller's; no CPU
 * fallback -- without a HIP device every call fails.
 */
#ifndef PGRC_MEM_H
#define PGRC_MEM_H

#include <stddef.h>
#include <stdint.h>

#include "pgrc_match.h"
#include "pgrc_varlen.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgrc_mem_ctx pgrc_mem_ctx;

/* TextMatch (matching/TextMatchers.h:10-16) */
typedef struct {
    uint64_t pos_src;  /* posSrcText */
    uint64_t length;
    uint64_t pos_dest; /* posDestText, in the coordinates of the text handed to pgrc_mem_match_texts */
} pgrc_text_match;

/* CopMEMMatcher(srcText, srcLength, targetMatchLength, minMatchLength) (CopMEMMatcher.cpp:571-591).
 * ctor_min_match_len: UINT32_MAX or >= target_match_len (what SimplePgMatcher passes; smaller values change K and
 * are not supported).  24 <= target_match_len <= 255. */
int pgrc_mem_create(uint32_t target_match_len, uint32_t ctor_min_match_len, int32_t device, pgrc_mem_ctx **out);
void pgrc_mem_destroy(pgrc_mem_ctx *ctx);
const char *pgrc_mem_last_error(const pgrc_mem_ctx *ctx);

/* The source text (ACGT): packed to HBM and indexed (the constructor's processRef, :176-231, serial semantics).
 * The pointer is borrowed until the context is destroyed or another source is set (like CopMEMMatcher::start1). */
int pgrc_mem_set_src_ascii(pgrc_mem_ctx *ctx, const char *src, uint64_t n);

/* matchTexts (:604-622).  dest is the text as the reference hands it over (SimplePgMatcher reverse-complements it
 * first when revComplMatching, SimplePgMatcher.cpp:31-41); it may contain 'N'.  With dest_is_src the library uses
 * its own copy of the source (or its reverse complement) on the device and dest is only read on the host.
 * *matches is malloc'ed (free with pgrc_mem_free_matches), discovery order. */
int pgrc_mem_match_texts(pgrc_mem_ctx *ctx, const char *dest, uint64_t n2, int dest_is_src, int rev_compl_matching,
                         uint32_t min_match_len, pgrc_text_match **matches, uint64_t *count);
void pgrc_mem_free_matches(pgrc_text_match *matches);

/* The same two calls for texts that are ALREADY IN HBM as ASCII, on the context's device: what pgrc_asm_text_device
 * (pgrc_assemble.h) returns.  The assembled pseudogenomes then reach SimplePgMatcher::matchPgsInPg's stage
 * (matching/SimplePgMatcher.cpp:175-206) without a trip to the host and back; only the matches, the two small streams per
 * text and the coded block come down.  Host and device forms mix freely: a device source with host
 * destinations and the reverse.  The texts may start at any byte address and must be complete when the call is made (no
 * kernel still writing them on another stream); they are read only while the call runs.
 *
 * pgrc_mem_set_src_device: pgrc_mem_set_src_ascii over d_ascii[0 .. n) (ACGT).  The text is packed into the context's own
 * words and indexed; nothing is borrowed -- the assembler may run again at once.  Same codes and messages as the host form
 * (PGRC_E_SYMBOL for a symbol outside ACGT, ...), and it forgets the remembered destination and the mapped slots as that does.
 *
 * pgrc_mem_match_texts_device: the destination in its FORWARD orientation, as assembled (it may contain 'N').  With
 * rev_compl_matching the library reverse-complements it on the device while packing it (the reference's complement table:
 * N stays N), so the matches, their coordinates and their order are those that pgrc_mem_match_texts returns for the
 * host-reversed text, and pgrc_mem_mark_and_remove, _resident and pgrc_mem_encode_mapped follow as after that call.  With
 * dest_is_src the library uses its own copy of the source; d_dest_ascii is not read and may be NULL.  Errors as in the host
 * form (PGRC_E_SYMBOL for a symbol outside ACGNT -- except in a text shorter than the K-mer, which is accepted but not
 * remembered --, PGRC_E_PARAM for dest_is_src with another length, a too long text, min_match_len < K; PGRC_E_STATE without
 * a source).
 *
 * Both: PGRC_E_PARAM for a pointer that is not device memory of the context's device (hipPointerGetAttributes). */
int pgrc_mem_set_src_device(pgrc_mem_ctx *ctx, const void *d_ascii, uint64_t n);
int pgrc_mem_match_texts_device(pgrc_mem_ctx *ctx, const void *d_dest_ascii, uint64_t n2, int dest_is_src, int rev_compl_matching,
                                uint32_t min_match_len, pgrc_text_match **matches, uint64_t *count);

/* markAndRemoveExactMatches (matching/SimplePgMatcher.cpp:69-148), the second half of SimplePgMatcher::matchPgsInPg, on
 * the device: the matches are normalised (correctDestPositionDueToRevComplMatching, :58-61;
 * resolveMappingCollisionsInTheSameText, :157-171), sorted, made unique and walked greedily; every kept match becomes one
 * '%' in the text, one entry of the offsets stream (4 bytes when the source length <= UINT32_MAX, else 8, little endian)
 * and one byte-frugal value of the lengths stream, which leads with min_match_len.
 *
 * It maps the destination of the LAST SUCCESSFUL pgrc_mem_match_texts of this context, which is still packed in HBM (no
 * text is uploaded): the context remembers that call's n2, dest_is_src and rev_compl_matching (pgrc_mem_match_texts_device
 * counts as that call).  pgrc_mem_set_src_ascii, pgrc_mem_set_src_device and a failed pgrc_mem_match_texts forget them
 * (PGRC_E_STATE here).  The mapped text is the destination in its forward
 * orientation, i.e. destPg itself, not the reverse complement that was matched.  A destination shorter than the index's
 * K-mer has no window to match, but pgrc_mem_match_texts still packs it to HBM so that it can be mapped.  One exception:
 * such a short destination that holds a symbol outside ACGNT is accepted by pgrc_mem_match_texts as it always was (no
 * window reads it), but it is not remembered: PGRC_E_STATE here.
 *
 * matches: a host array in matchTexts' coordinates, normally what that call returned (it need not be: symbols are not
 * compared).  min_match_len: UINT32_MAX = the target match length.  mapped_out: the caller's buffer (pageable or
 * page-locked) of mapped_cap >= n2 bytes; it may be the destination string's own storage -- the library does not read the
 * host text.  The two streams come in one block the library allocates; pgrc_mem_free_mapping frees it and clears *out.
 * count == 0: the text unchanged, an empty map_off and a map_len that holds min_match_len alone (what the reference
 * writes when a matcher exists and finds nothing).
 *
 * PGRC_E_PARAM (with *out cleared, the context still usable): mapped_cap < n2; a match with length 0, with
 * pos_src + length > the source length or with pos_dest + length > n2; min_match_len == 0.
 *
 * Out of scope: the case without a matcher (a source shorter than the target length: SimplePgMatcher writes the text
 * and no streams) and the entropy coding of the three results; both stay with the caller. */
typedef struct {
    uint64_t mapped_len;                      /* bytes written to mapped_out */
    uint64_t marks, unique_matches, matched_symbols; /* unique_matches: different normalised (dest, src, length) triples */
    uint8_t *map_off; uint64_t map_off_bytes; /* marks x 4 or 8 */
    uint8_t *map_len; uint64_t map_len_bytes; /* leads with min_match_len */
} pgrc_mem_mapping;
int pgrc_mem_mark_and_remove(pgrc_mem_ctx *ctx, const pgrc_text_match *matches, uint64_t count, uint32_t min_match_len,
                             char *mapped_out, uint64_t mapped_cap, pgrc_mem_mapping *out);
void pgrc_mem_free_mapping(pgrc_mem_mapping *m);

/* The same mapping with the mapped text KEPT IN HBM, for the variable-length DNA coder (pgrc_varlen.h) that the reference
 * runs over the joined mapped texts HQ | LQ | N before LZMA / PPMd (SimplePgMatcher::matchPgsInPg,
 * matching/SimplePgMatcher.cpp:208-231): the text then crosses the link at about 0.3 byte a symbol instead of one.
 *
 * pgrc_mem_mark_and_remove_resident is pgrc_mem_mark_and_remove without mapped_out: the mapped text stays in the
 * context's slot `part` (0 HQ, 1 LQ, 2 N; anything else is PGRC_E_PARAM), the two streams and the counters come back as
 * before, out->mapped_len is the slot's length.  A failed call leaves the slot unset.
 *
 * pgrc_mem_encode_mapped codes the slots 0 | 1 | 2 as ONE text with `v` into coded_out (host, cap bytes;
 * pgrc_varlen_bound(sum of the lengths) always suffices) and returns the three mapped lengths, which the caller writes as
 * pgsLen.  An unset N slot is an empty part; an unset HQ or LQ slot is PGRC_E_STATE; a coder on another device is
 * PGRC_E_PARAM; the coder's own failures (PGRC_E_SYMBOL, a cap below the coded length: PGRC_E_PARAM with *coded_len = the
 * length needed) come back as they are.  pgrc_mem_set_src_ascii forgets the slots.  The case without a matcher (a source
 * shorter than the target length) stays with the caller, who codes the texts with pgrc_varlen_encode directly. */
int pgrc_mem_mark_and_remove_resident(pgrc_mem_ctx *ctx, const pgrc_text_match *matches, uint64_t count, uint32_t min_match_len,
                                      int32_t part, pgrc_mem_mapping *out);
int pgrc_mem_encode_mapped(pgrc_mem_ctx *ctx, pgrc_varlen *v, void *coded_out, uint64_t cap, uint64_t *coded_len, uint64_t lens[3]);

/* introspection (tests, bench) */
typedef struct {
    uint64_t probes;       /* destination windows hashed */
    uint64_t events;       /* (window, index entry) pairs with equal K-mers */
    uint64_t stale_lookups;/* events that needed the stale-register emulation on the host (for a text without a host copy it
                            * fetches the few bytes it looks at from the packed text on the device) */
    float ms_index, ms_probe, ms_sort, ms_extend;
    float ms_host;         /* compaction + download of the matches */
    float ms_replay;       /* the sequential rules on the device, all rounds (host clock) */
    uint32_t replay_rounds;/* passes over the event blocks until every block had seen the last match before it */
    uint32_t event_blocks; /* blocks of 256 windows that hold events */
} pgrc_mem_counters;
int pgrc_mem_get_counters(pgrc_mem_ctx *ctx, pgrc_mem_counters *out);
/* phases of the last pgrc_mem_mark_and_remove in milliseconds: [0] normalise + sort + unique, [1] the greedy path,
 * [2] marks and both streams, [3] the text kernel (device events), [4] the downloads (host clock) */
int pgrc_mem_mapping_timing(pgrc_mem_ctx *ctx, float ms[5]);

#ifdef __cplusplus
}
#endif
#endif /* PGRC_MEM_H */
