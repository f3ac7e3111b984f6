// decctx.h -- the decode context of include/pgrc_decode.h and the helpers its sources share: decode.hip (the reads
// rebuild), restore.hip (the restore of the matched pseudogenomes), pairpos.hip (the pair positions of the paired ORD mode),
// pairorder.hip (the pair order of the paired non-ORD mode) and listarchive.hip (the archive form of a list's mismatch streams).
#pragma once

#include <string.h>

#include <algorithm>
#include <string>

#include "ctx.h"
#include "pgrc_decode.h"
#include "scanops.h"

#define DEC_TPB 256
#define DEC_TEXT_PAD 64         // zero bytes after the text: aligned 16-byte loads past a window's end stay inside
#define DEC_STAGE_BYTES (64ull << 20)

// error flags of the device checks (the word at pgrc_decode_ctx::flag)
#define DEC_F_WINDOW 1u         // a window reaches past the text end
#define DEC_F_INDEX 2u          // an rlIdx / rank out of range
#define DEC_F_MISOFF 4u         // a mismatch offset outside the read
#define DEC_F_MISSYM 8u         // a mismatch code outside its form's range
#define DEC_F_NOPOS 16u         // a row needs the positions of a list that has none

struct pgrc_decode_ctx : PgrcDev {
    uint32_t L = 0;
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_made[2]{}, ev_copied[2]{}, ev_k0[2]{}, ev_a{}, ev_b{};
    uint8_t *stage[2]{};        // pinned staging (uploads and downloads of pageable memory)
    DevBuf chunk[2];            // device chunks of rows
    DevBuf text, flag, scratch;
    uint64_t text_len = 0;
    bool have_text = false;
    struct List {
        DevBuf pos, rc, mcum, moff, msym, raw;
        uint64_t n = 0, nmis = 0;
        bool has_pos = false, has_rc = false, has_mis = false;
        uint32_t form = 0;
        char order[5];
        uint64_t text_base = 0;
    } lst[3];
    uint32_t nl = 0;
    bool have_order = false;
    pgrc_decode_order ord{};
    DevBuf rl_order, org2pos, rank;
    pgrc_decode_timing tm{};
    // pgrc_decode_set_mapped_text (restore.hip): the parts of the restored text, its scratch (kept for the next call,
    // freed with the context) and its timing
    bool have_parts = false;
    uint64_t part_len[3] = {};
    DevBuf rs_mapped, rs_marks, rs_vals, rs_ptr, rs_bsum;   // the mapped parts and streams; per-mark arrays; values; pointers; block counts
    DevBuf rs_coded, rs_join;   // pgrc_decode_set_mapped_text_coded: the coded bytes and the joined text they decode to
    pgrc_decode_restore_timing rtm{};
    // the pair-position coding (pairpos.hip): the uploaded input, the sort's records (and values, W = 8) in turn, per-rank
    // and per-far-pair arrays, the device-side output, scan scratch; pp_sort: the scratch of radix.hip's sort
    DevBuf pp_in, pp_rec[2], pp_val[2], pp_rank, pp_far, pp_out, pp_bsum;
    DevBuf pp_sort;
    hipEvent_t pp_ev[6]{};
    bool have_pp_timing = false;
    pgrc_pairpos_timing ptm{};
    // the pair-order coding (pairorder.hip): the joined orgIdx, rev, per-entry and per-pair arrays, the device-side streams,
    // scan scratch and the two error words
    DevBuf po_in, po_rev, po_ent, po_pair, po_out, po_bsum;
    hipEvent_t po_ev[11]{};
    bool have_po_timing = false;
    pgrc_pairorder_timing potm{};
    // the archive form of the mismatch streams (listarchive.hip): the uploaded streams, the flag scan, the counts (decode),
    // the mismatch-list starts (encode), the count matrix and its scan scratch, the per-count words, the device-side block
    DevBuf la_in, la_inc, la_cnt, la_mcum, la_mat, la_fold, la_small, la_out;
    hipEvent_t la_ev[8]{};
    bool have_la_timing = false;
    pgrc_list_archive_timing latm{};
};

// pairpos.hip: the file-major positions of `s` as n_total u64 at d_out (device, on d->stream; synchronised on return);
// fills d->ptm but for ms_download / ms_call
int pgrc_pairpos_decode_device(pgrc_decode_ctx *d, const pgrc_pairpos_streams *s, uint64_t *d_out);
int pgrc_pairpos_check_streams(pgrc_decode_ctx *d, const pgrc_pairpos_streams *s);   // the checks that need no device (PGRC_E_PARAM)
void pgrc_pairpos_release(pgrc_decode_ctx *d);     // the buffers and events above (pgrc_decode_destroy)
void pgrc_pairorder_release(pgrc_decode_ctx *d);   // pairorder.hip: its buffers and events (pgrc_decode_destroy)
void pgrc_la_release(pgrc_decode_ctx *d);          // listarchive.hip: its buffers and events (pgrc_decode_destroy)
// listarchive.hip: the mismatch tables of list `l` (mcum, moff, msym, nmis) from the archive-form streams `s`, on d->stream;
// device-side findings (DEC_F_MISOFF, DEC_F_MISSYM) go to d->flag, which the caller reads (pgrc_decode_add_list_archive)
int pgrc_la_tables(pgrc_decode_ctx *d, pgrc_decode_ctx::List &l, const pgrc_list_archive_streams *s);
// decode.hip: pgrc_decode_add_list, with the mismatches from `arch` when it is given
int pgrc_dec_add_list(pgrc_decode_ctx *d, const pgrc_decode_list *a, const pgrc_list_archive_streams *arch);

static int dec_fail(pgrc_decode_ctx *d, int code, const std::string &msg) {
    d->err = msg;
    return code;
}

static void dec_free(DevBuf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

static float dec_elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return ms;
}

static int dec_clear_err(pgrc_decode_ctx *d) {
    HIP_TRY(d, hipMemsetAsync(d->flag.p, 0, 4, d->stream));
    return PGRC_OK;
}

// host -> device through the two pinned staging buffers: the copy of one overlaps the host's fill of the other
static int dec_upload(pgrc_decode_ctx *d, void *d_dst, const void *h_src, uint64_t bytes) {
    const uint8_t *src = (const uint8_t *)h_src;
    uint8_t *dst = (uint8_t *)d_dst;
    int k = 0;
    for (uint64_t o = 0; o < bytes; o += DEC_STAGE_BYTES, k ^= 1) {
        const uint64_t c = std::min<uint64_t>(DEC_STAGE_BYTES, bytes - o);
        HIP_TRY(d, hipEventSynchronize(d->ev_copied[k]));
        memcpy(d->stage[k], src + o, c);
        HIP_TRY(d, hipMemcpyAsync(dst + o, d->stage[k], c, hipMemcpyHostToDevice, d->stream));
        HIP_TRY(d, hipEventRecord(d->ev_copied[k], d->stream));
    }
    return PGRC_OK;
}

// the same from memory that may be page-locked: then the copy engine reads it where it is
static int dec_upload_host(pgrc_decode_ctx *d, void *dst, const void *src, uint64_t bytes) {
    if (!bytes || !pgrc_host_pinned(src)) return dec_upload(d, dst, src, bytes);
    HIP_TRY(d, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, d->stream));
    return PGRC_OK;
}

// ------------------------------------------------------------------------------------------------ scans (u64 results)
struct XfU8 { const uint8_t *p; __device__ uint64_t operator()(uint64_t i) const { return p[i]; } };
struct XfU16 { const uint16_t *p; __device__ uint64_t operator()(uint64_t i) const { return p[i]; } };
struct XfBelow { const uint64_t *p; uint64_t lim; __device__ uint64_t operator()(uint64_t i) const { return p[i] < lim ? 1u : 0u; } };

// out[i] = base_val + (INCLUSIVE ? sum of xf(0..i) : sum of xf(0..i-1)); the exclusive form also writes out[n] = base_val + total
template <bool INCLUSIVE, typename Xf>
static int dec_scan(pgrc_decode_ctx *d, Xf xf, uint64_t n, uint64_t base_val, uint64_t *d_out) {
    int e;
    if ((e = pgrc_buf_unpooled(d, d->scratch, sco_scratch_elems(n) * sizeof(uint64_t)))) return e;
    HIP_TRY(d, (sco_device_scan<INCLUSIVE, true>(d->stream, xf, n, ScoPlus{}, (uint64_t)0, base_val, ScoStore<uint64_t>{d_out}, (uint64_t *)d->scratch.p)));
    return PGRC_OK;
}

// complementsLut (helper.cpp:243-262): IUPAC complements of both cases to upper case, every other byte to 0
static __device__ __forceinline__ uint8_t dec_complement(uint32_t c) {
    const uint32_t u = c & 0xDFu;   // upper case (only letters are mapped)
    if (c < 'A' || (c > 'Z' && c < 'a') || c > 'z') return 0;
    switch (u) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    case 'N': return 'N';
    case 'U': return 'A';
    case 'Y': return 'R';
    case 'R': return 'Y';
    case 'K': return 'M';
    case 'M': return 'K';
    case 'B': return 'V';
    case 'V': return 'B';
    case 'D': return 'H';
    case 'H': return 'D';
    default: return 0;
    }
}
