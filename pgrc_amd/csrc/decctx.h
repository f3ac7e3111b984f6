// decctx.h -- the decode context of include/pgrc_decode.h and the helpers its sources share: decode.hip (the reads
// rebuild) and restore.hip (the restore of the matched pseudogenomes).  What it shares with the other stages -- the stream, the
// staging buffers, the copies through them -- is stagectx.h's PgrcStage.  The exported entry points of the three list codings
// (pairpos.hip, pairorder.hip, listarchive.hip) take a decode context too: it holds one state of each (codingctx.h), which
// they hand to coders that know the stage and that state alone.
#pragma once

#include "codingctx.h"

#define DEC_TPB 256
#define DEC_TEXT_PAD 64         // zero bytes after the text: aligned 16-byte loads past a window's end stay inside

// error flags of the device checks (the word at pgrc_decode_ctx::flag)
#define DEC_F_WINDOW 1u         // a window reaches past the text end
#define DEC_F_INDEX 2u          // an rlIdx / rank out of range
#define DEC_F_MISOFF 4u         // a mismatch offset outside the read
#define DEC_F_MISSYM 8u         // a mismatch code outside its form's range
#define DEC_F_NOPOS 16u         // a row needs the positions of a list that has none

struct pgrc_decode_ctx : PgrcStage {
    uint32_t L = 0;
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_made[2]{}, ev_k0[2]{}, ev_a{}, ev_b{};
    DevBuf chunk[2];            // device chunks of rows
    DevBuf text;
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
    // the list codings behind pgrc_pairpos_*, pgrc_pairorder_* and pgrc_list_archive_* (codingctx.h)
    PgrcPairPos pp;
    PgrcPairOrder po;
    PgrcPairOrderDec pod;
    PgrcListArchive la;
};

// decode.hip: pgrc_decode_create without a read length, for the assembly (pgasm.hip), which keeps a decode context for the
// text it holds and gives every call its own length
int pgrc_decode_create_on(int32_t device, pgrc_decode_ctx **out);
// pairpos.hip: the file-major positions of `s` as n_total u64 at d_out (device, on d->stream; synchronised on return);
// fills d->pp.tm but for ms_download / ms_call
int pgrc_pairpos_decode_device(pgrc_decode_ctx *d, const pgrc_pairpos_streams *s, uint64_t *d_out);
int pgrc_pairpos_check_streams(PgrcStage *d, const pgrc_pairpos_streams *s);   // the checks that need no device (PGRC_E_PARAM)
// pairorder.hip: rlIdxOrder of `s` as n_total u32 at d_out (device, on d->stream; synchronised on return, every device-side
// finding already turned into PGRC_E_PARAM); fills d->pod.tm but for ms_download / ms_call
int pgrc_pairorder_decode_device(pgrc_decode_ctx *d, const pgrc_pairorder_streams *s, uint32_t *d_out);
int pgrc_pairorder_check_streams(PgrcStage *d, const pgrc_pairorder_streams *s);   // the checks that need no device (PGRC_E_PARAM)
// listarchive.hip: the mismatch tables of list `l` (mcum, moff, msym, nmis) from the archive-form streams `s`, on d->stream with d->la;
// device-side findings (DEC_F_MISOFF, DEC_F_MISSYM) go to d->flag, which the caller reads (pgrc_decode_add_list_archive)
int pgrc_la_tables(pgrc_decode_ctx *d, pgrc_decode_ctx::List &l, const pgrc_list_archive_streams *s);
// decode.hip: pgrc_decode_add_list, with the mismatches from `arch` when it is given
int pgrc_dec_add_list(pgrc_decode_ctx *d, const pgrc_decode_list *a, const pgrc_list_archive_streams *arch);

// ------------------------------------------------------------------------------------------------ scans (u64 results)
struct XfU8 { const uint8_t *p; __device__ uint64_t operator()(uint64_t i) const { return p[i]; } };
struct XfU16 { const uint16_t *p; __device__ uint64_t operator()(uint64_t i) const { return p[i]; } };
struct XfBelow { const uint64_t *p; uint64_t lim; __device__ uint64_t operator()(uint64_t i) const { return p[i] < lim ? 1u : 0u; } };

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
