/*
 * pgrc_varlen.h -- C ABI of libpgrc_match.so, part 6: the variable-length DNA coder on MI355X.
 *
 * Drop-in boundary: PgHelpers::VarLenDNACoder (coders/VarLenDNACoder.{h,cpp}), the static book of up to 256 codes of 0-4
 * symbols, one output byte per code, that SimplePgMatcher::matchPgsInPg pushes the joined mapped pseudogenomes through
 * before LZMA / PPMd see them (matching/SimplePgMatcher.cpp:208-231) and that restoreMatchedPgs undoes (:259-351).
 *
 * Result semantics = VarLenDNACoder::encode (:55-104) and ::decode (:106-120), byte for byte, payload only: the two
 * header bytes and the book that Compress writes in front of the payload (:135-147) stay with the caller, who has them.
 * The book is an INPUT: the bytes VarLenDNACoder::writeBook produces (every code followed by '\n', the last '\n'
 * replaced by NUL), i.e. what stands behind the two header bytes of a coded stream.
 *
 * encode, restated: at position pos, with the four bytes from pos on as a little-endian word masked to 27 bits (bytes
 * past the end are zero), the longest rung r in 4, 3, 2 with at least r bytes left whose r-byte key is in the book is
 * emitted and pos += r; else the one-symbol code of src[pos] (whatever the look-up gives) and pos += 1.  For a text
 * shorter than 4 the reference's unsigned `srcLen - 4` wraps; that case is defined here as the same rule from position 0.
 *
 * Device buffers: the coder works on a HIP stream of its own, which is not ordered with the caller's streams (the null
 * stream included).  Every device part, coded stream and output handed to a call must be COMPLETE before the call: whatever
 * the caller has queued that writes a source, or reads or writes an output, has finished (hipStreamSynchronize of that
 * stream, or a wait of the same effect).  On return every result is complete: the call synchronises its own stream.
 *
 * Same conventions as pgrc_match.h: 0 = success, PGRC_E_* otherwise; buffers stay the caller's; all lengths are
 * uint64_t; no CPU fallback -- without a HIP device every call fails.
 */
#ifndef PGRC_VARLEN_H
#define PGRC_VARLEN_H

#include <stddef.h>
#include <stdint.h>

#include "pgrc_match.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgrc_varlen pgrc_varlen;

/* book: the writeBook form, book_bytes with or without the trailing NUL.  device: HIP ordinal, -1 = current.
 * PGRC_E_PARAM: more than 256 codes; a code longer than 4 bytes; code 0 is not one symbol; a symbol of the book without
 * a one-symbol code; two symbols of the book that share their low three bits (the reference's 27-bit key cannot tell
 * them apart in the fourth place); a symbol whose low three bits are 0, such as 'H' or 'P' (in the fourth place that key
 * cannot tell it from no byte at all: a three-symbol code would be emitted with a step of four, and the stream would not
 * decode to its input).  The checks come before the device is touched. */
int pgrc_varlen_create(const void *book, uint64_t book_bytes, int32_t device, pgrc_varlen **out);
void pgrc_varlen_destroy(pgrc_varlen *v);
const char *pgrc_varlen_last_error(const pgrc_varlen *v);   /* NULL: the last failed create of this thread */

/* the coded length of n symbols at worst: one code per symbol */
uint64_t pgrc_varlen_bound(uint64_t n);

/* One part of the source text: a host pointer (pageable or page-locked), or a device pointer on the coder's device. */
typedef struct {
    const void *ptr;
    uint64_t len;
    int32_t on_device;
} pgrc_varlen_part;

/* Codes parts[0] | parts[1] | ... (n_parts <= 3: the joined text is HQ | LQ | N) as ONE text; a part may be empty, and a
 * look-up window may span two or three parts.  out: out_cap bytes on the host or (out_on_device) on the device.
 * PGRC_E_SYMBOL: a byte that is no symbol of the book (the reference would silently write a stream that does not decode
 * to its input); nothing usable is written.  PGRC_E_PARAM: out_cap below the coded length (nothing written; *coded_len
 * holds the length needed). */
int pgrc_varlen_encode(pgrc_varlen *v, const pgrc_varlen_part *parts, uint32_t n_parts, void *out, uint64_t out_cap,
                       int32_t out_on_device, uint64_t *coded_len);

/* Every coded byte appends its code's symbols (a byte at or beyond the book's number of codes appends nothing, like an
 * empty code).  out: expected_len bytes, host or device.  PGRC_E_PARAM: the total differs from expected_len (the
 * reference exits there); nothing is written. */
int pgrc_varlen_decode(pgrc_varlen *v, const void *coded, uint64_t coded_len, int32_t coded_on_device,
                       uint64_t expected_len, void *out, int32_t out_on_device);

/* the last encode or decode in milliseconds.  ms_upload / ms_download: host clock, 0 for device buffers; the three
 * phases: device events.  encode: the tile maps (pass 1), the two scans, the emit (pass 2); decode: the lengths, the
 * scan, the expansion. */
typedef struct {
    float ms_upload, ms_maps, ms_scan, ms_emit, ms_download, ms_call;
    uint64_t symbols, coded_bytes;
    int32_t was_decode;
} pgrc_varlen_times;
int pgrc_varlen_timing(pgrc_varlen *v, pgrc_varlen_times *out);

#ifdef __cplusplus
}
#endif
#endif /* PGRC_VARLEN_H */
