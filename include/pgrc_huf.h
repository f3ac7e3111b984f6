/*
 * pgrc_huf.h -- C ABI of libpgrc_huf.so: the Huffman mode of the reference's coder type 5 on MI355X.
 *
 * Drop-in boundary: FSECompress / FSEUncompress (coders/FSECoder.cpp:15-135) with FSECoderProps::HUF_MODE, i.e. what
 * getDefaultHufCoderProps (coders/PropsLibrary.cpp:48-50) selects: HUF_compress2 / HUF_decompress (coders/fse/huf_compress.c,
 * huf_decompress.c) over independent chunks.  The payload is what stands behind a stream's 17-byte header in an archive, the
 * four props bytes included.  What this coder writes, the unmodified reference reads; what the reference writes in this mode,
 * this coder reads.  The writer's choices differ from the reference's (its streams are not byte-identical to HUF_compress2's);
 * they are fixed, so that equal input gives equal output: tests/huf_util.py restates them, DESIGN.md 4.25 lists them.
 *
 * The format, restated:
 *   frame    4 props bytes: mode (0 = Huffman, 1 = FSE), blockSizeOrder, maxSymbolValue, tableLog (FSECoder.cpp:34-37; the last
 *            two are informative, :91-98).  Then, per chunk of 1 << blockSizeOrder source bytes (the last one shorter): a
 *            4-byte little-endian coded size and the coded chunk; the LAST chunk carries no size and takes the rest (:44-78,
 *            :104-132).  An empty source is the four props bytes.
 *   chunk    coded size 1: every byte of the chunk is that byte (:116-118, huf_decompress.c:1066).  Coded size = chunk
 *            length: the bytes as they are (:1065).  A larger size is damage (:1064).  Else: weight header, jump table, four
 *            streams.  This writer codes a chunk only when that is strictly shorter than the chunk, so the three cases
 *            never collide; a chunk under 12 bytes is never coded (huf_compress.c:565).
 *   header   HUF_readStats (entropy_common.c:154-215).  First byte h >= 128: h - 127 weights of 4 bits each follow, the
 *            first in the high half of a byte (:167-177).  h < 128: h bytes follow, an FSE table (FSE_readNCount, :40-144) at
 *            table log 5 or 6 and a two-state FSE stream of up to 255 weights (fse_decompress.c:178-238).  A weight is
 *            0 (absent) or tableLog + 1 - code length, below 12; the weight of the last present symbol is not stored: it
 *            is what brings the sum of 2^(weight - 1) to the next power of two, 2^tableLog (:196-207).  Weight 1 occurs an
 *            even number of times, at least twice (:210).  This writer uses the 4-bit form when the highest present symbol is
 *            <= 128 (the form cannot say more, huf_compress.c:140) and the FSE form above; where that does not fit into 127
 *            bytes it stores the chunk raw.
 *   codes    HUF_readDTableX1_wksp (huf_decompress.c:151-183): the table of 2^tableLog cells is filled by rising weight and,
 *            within a weight, by rising symbol, 2^(weight - 1) cells a symbol.  So the longest codes count up from 0, and every
 *            shorter length continues where the longer one ended, halved (HUF_buildCTable_wksp, huf_compress.c:390-407).
 *   streams  a jump table of three u16: the byte sizes of the first three streams (huf_compress.c:566-592); the four
 *            segments are (n + 3) / 4 source bytes each, the last one the rest (:557).  A stream holds its segment's codes
 *            from the LAST symbol (lowest bits of byte 0) to the first, a code's value with its low bit lowest, then one
 *            end-mark bit; the rest of the last byte is zero (:457-512, BIT_closeCStream).  A reader starts under the end
 *            mark and must end exactly at bit 0 with its segment full (huf_decompress.c:253-257, :348-349).
 *
 * Limits: the writer takes block_order 1 .. 17 (the reference's chunks end at 128 KiB, HUF_BLOCKSIZE_MAX) and table_log
 * 8 .. 11, 0 for the default 11 (256 symbols need 8; the reference's default is 11).  The reader takes block orders up to 17
 * and code lengths up to 12, which HUF_readStats allows.
 *
 * Device buffers: as in pgrc_varlen.h.  The coder works on a HIP stream of its own; a device source, coded stream or output
 * handed to a call must be COMPLETE before the call, and on return every result is complete.
 *
 * Same conventions as pgrc_match.h: 0 = success, PGRC_E_* otherwise; buffers stay the caller's; all lengths are
 * uint64_t; no CPU fallback -- without a HIP device every call fails.  Argument checks come before the device is touched.
 */
#ifndef PGRC_HUF_H
#define PGRC_HUF_H

#include <stddef.h>
#include <stdint.h>

#include "pgrc_match.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgrc_huf pgrc_huf;

#define PGRC_HUF_ORDER_MAX 17
#define PGRC_HUF_TABLE_LOG_MIN 8
#define PGRC_HUF_TABLE_LOG_MAX 11

/* device: HIP ordinal, -1 = current */
int pgrc_huf_create(int32_t device, pgrc_huf **out);
void pgrc_huf_destroy(pgrc_huf *h);
const char *pgrc_huf_last_error(const pgrc_huf *h);   /* NULL: the last failed create of this thread */

/* the coded length of n bytes at worst: the props, every chunk raw, a size in front of all but the last; 0 for a
 * block_order outside 1 .. 17 */
uint64_t pgrc_huf_bound(uint64_t n, uint32_t block_order);

/* src: n bytes on the host (pageable or page-locked) or (src_on_device) on the coder's device.  out: out_cap bytes, host or
 * device.  PGRC_E_PARAM: a NULL argument, block_order outside 1 .. 17, table_log other than 0 or 8 .. 11, or out_cap below
 * the coded length (nothing written; *coded_len holds the length needed, and the handle stays usable).  The call never
 * refuses for size: a frame longer than its source (every chunk raw) is the caller's to store as it is. */
int pgrc_huf_encode(pgrc_huf *h, const void *src, uint64_t n, int32_t src_on_device, uint32_t block_order, uint32_t table_log,
                    void *out, uint64_t out_cap, int32_t out_on_device, uint64_t *coded_len);

/* out: expected_len bytes, host or device.  PGRC_E_PARAM with a message: a frame in FSE mode or with a block order above 17,
 * and every damaged stream (a frame cut short, a chunk size past the end or above the chunk's length, a weight header that
 * is no valid one, a jump table beyond the chunk, a stream that ends early or late).  Every read is checked against the
 * chunk and every write against the segment, so damage never reaches beyond the buffers; nothing is written behind
 * expected_len, and to a host `out` nothing at all. */
int pgrc_huf_decode(pgrc_huf *h, const void *coded, uint64_t coded_len, int32_t coded_on_device, uint64_t expected_len, void *out,
                    int32_t out_on_device);

/* the last encode or decode in milliseconds.  ms_upload / ms_download: host clock, 0 for device buffers; the phases: device
 * events.  encode: the histograms, code tables and headers; the streams; the scan of the sizes and the compaction.  decode:
 * the walk over the sizes (ms_tables); the headers, tables and streams (ms_emit); ms_compact is 0. */
typedef struct {
    float ms_upload, ms_tables, ms_emit, ms_compact, ms_download, ms_call;
    uint64_t bytes, coded_bytes;
    uint32_t chunks, huf_chunks, rle_chunks, raw_chunks;
    int32_t was_decode;
} pgrc_huf_times;
int pgrc_huf_timing(pgrc_huf *h, pgrc_huf_times *out);

#ifdef __cplusplus
}
#endif
#endif /* PGRC_HUF_H */
