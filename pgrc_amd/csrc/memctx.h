// memctx.h -- the context behind include/pgrc_mem.h, shared by the matcher (mem.hip) and the mapping of its matches (pgmap.hip).
//
// The context is a base matcher context (the packed source, its reverse complement, the seed index, the device, the stream and
// the ONE error text: pgrc_mem_last_error returns base->err) and the parts below.  mem.hip owns the source, the destination, the
// events, the runs and the replay; pgmap.hip owns the mapping's buffers and the resident mapped texts.  Of a finished match
// pgmap.hip reads three things and nothing else: the destination part (MemDest), the radix sort's scratch (MemEvents::tmp, which
// its own sorts reuse) and base->txt (the packed source, which is the destination of a dest_is_src call).
#pragma once

#include <stddef.h>

#include <string>

#include "ctx.h"
#include "pgrc_mem.h"

// The source text as the last pgrc_mem_set_src_* left it.  Its words, reverse complement and index are the base context's.
struct MemSource {
    uint32_t L = 0;                   // the target match length the context was made with
    int K = 0, k1 = 0, k2 = 0, LK2 = 0, KLK24 = 0;
    const char *text = nullptr;       // borrowed host text; null after pgrc_mem_set_src_device (the packed words are all there is)
    uint64_t N = 0;
    bool have = false;
};

// The destination of the last successful pgrc_mem_match_texts, as pgrc_mem_mark_and_remove maps it (pgmap.hip): packed in
// base->txt.pg2[0] (dest_is_src) or in words / nmap, which then hold the text as it was handed over (the reverse complement when
// rev_compl).
struct MemDest {
    DevBuf words, nmap;               // 2-bit words and one N bit per symbol, PGRC_PG_PAD_WORDS of zeros behind either
    DevBuf stage, flag;               // one chunk of a host text on its way up; bit 0 a symbol outside ACGNT, bit 1 an N
    bool ready = false, dest_is_src = false, rev_compl = false, has_n = false;
    uint64_t n2 = 0;
    DevBufList bufs() { return {&words, &nmap, &stage, &flag}; }
    // a match call has succeeded: its destination is resident and can be mapped
    int done(uint64_t N2, bool is_src, bool rc, bool n) {
        ready = true;
        n2 = N2;
        dest_is_src = is_src;
        rev_compl = rc;
        has_n = n;
        return PGRC_OK;
    }
};

// The events: the (window, source position) pairs whose K-mers are equal, as the probe writes and the first sort orders them
struct MemEvents {
    DevBuf cursor;                    // u64: events written (counted past the capacity: the probe then runs again)
    DevBuf evk[2], evv[2];            // (window << 4 | bucket order) and source position: the sort's ping-pong
    DevBuf tmp;                       // scratch of every radix sort of this context, pgmap.hip's included
    DevBufList bufs() { return {&cursor, &evk[0], &evk[1], &evv[0], &evv[1], &tmp}; }
};

// The runs: events by (diagonal, window), numbered by the maximal match they lie in, and that match's extents
struct MemRuns {
    DevBuf skey[2], sidx[2];          // diagonal keys and event indices: the second sort's ping-pong
    // Two u32 per event that serve one phase after the other (the earlier tenant is dead when the next one writes):
    //   mark   runs: 1 = the event starts a run     replay: 1 = the event leads an event block   emit: accepted events up to it
    //   rank   runs: inclusive sum of the run marks   replay, emit: inclusive sum of the leader marks (event block + 1)
    DevBuf mark, rank;
    DevBuf rstart, rend, rdend;       // per run: first source symbol, source and destination position after the match
    DevBuf orun, oflag;               // per event (in the reference's order): its run, its MF_* flags
    DevBuf scan;                      // block folds of the scans over the events (scanops.h)
    DevBufList bufs() { return {&skey[0], &skey[1], &sidx[0], &sidx[1], &mark, &rank, &rstart, &rend, &rdend, &orun, &oflag, &scan}; }
    uint32_t *run_first() const { return (uint32_t *)mark.p; }
    uint32_t *run_id() const { return (uint32_t *)rank.p; }
    uint32_t *block_lead() const { return (uint32_t *)mark.p; }
    uint32_t *block_id() const { return (uint32_t *)rank.p; }
    uint32_t *emit_slot() const { return (uint32_t *)mark.p; }
    uint32_t *folds() const { return (uint32_t *)scan.p; }
};

// The few words the replay and the host exchange (MemReplay::small: one of these, cleared whole per call)
struct MemSmall {
    uint32_t changed;                 // a block was replayed in this round
    uint32_t first_stale;             // smallest event index with outcome MO_STALE
    uint32_t nstale;                  // events with a side context outside a text
    uint32_t unused;
    uint64_t range[2];                // [lo, hi) of the events of a range of windows (k_mem_find_range)
    uint64_t spare[4];                // (the block has always been 64 bytes)
};
static_assert(sizeof(MemSmall) == 64 && offsetof(MemSmall, range) == 16, "the kernels get pointers into this block");

// The replay: outcome per event, the event blocks' state, the matches on their way down
struct MemReplay {
    DevBuf outc;                      // MO_* per event
    DevBuf ebstart, ebin, ebout, ebinc;   // per event block: MemReplayArgs (mem.hip)
    DevBuf small;                     // one MemSmall
    DevBuf match;                     // the accepted events as pgrc_text_match, in discovery order
    DevBufList bufs() { return {&outc, &ebstart, &ebin, &ebout, &ebinc, &small, &match}; }
    template <typename T>
    T *small_at(size_t offset) const { return (T *)((char *)small.p + offset); }
    uint32_t *changed() const { return small_at<uint32_t>(offsetof(MemSmall, changed)); }
    uint32_t *first_stale() const { return small_at<uint32_t>(offsetof(MemSmall, first_stale)); }
    uint32_t *nstale() const { return small_at<uint32_t>(offsetof(MemSmall, nstale)); }
    uint64_t *range() const { return small_at<uint64_t>(offsetof(MemSmall, range)); }
};

// The mapping (pgmap.hip): what one pgrc_mem_mark_and_remove call works in, phase by phase
struct PmBufs {
    DevBuf in, f[3];                  // the matches as handed over; dst, src, len after the corrections
    DevBuf key[2], idx[2], flag;      // the three sorts' ping-pong; bit 0 enters the greedy pass, bit 1 differs from its predecessor
    DevBuf slot;                      // u32, sort phase: [n] greedy slots, [n] unique counts; path phase: [nu] slots of the kept matches
    DevBuf u[4];                      // the matches of the greedy pass: dst, src, e = dst + len, t = e - min_len
    DevBuf pmax, jump[2], kept;       // prefix maxima of t; next() pointers, doubling; 1 = on the path
    DevBuf m[3];                      // the marks: dst, src, e of the kept matches
    DevBuf dp, len, nb, cum, nbpos, mp, off, lens;   // per mark: d', L', width of its length value, their sums, its place; the two streams
    DevBuf out;                       // the mapped text of a call that downloads it
    DevBuf fold;                      // block folds of the scans, u32 or u64 as the scan needs
    DevBuf small;                     // u32: PM_BAD_* found by k_pm_norm
    PhaseEvents<5> ev;                // (created on first use)
    float ms[5] = {0, 0, 0, 0, 0};    // normalise + sort, path, streams, text, download
    DevBufList bufs() {
        return {&in, &f[0], &f[1], &f[2], &key[0], &key[1], &idx[0], &idx[1], &flag, &slot, &u[0], &u[1], &u[2], &u[3], &pmax, &jump[0], &jump[1], &kept,
                &m[0], &m[1], &m[2], &dp, &len, &nb, &cum, &nbpos, &mp, &off, &lens, &out, &fold, &small};
    }
};

// The mapped texts that pgrc_mem_mark_and_remove_resident left in HBM, slot 0 HQ, 1 LQ, 2 N: what pgrc_mem_encode_mapped codes
// as one text (a new source forgets them)
struct PmResident {
    DevBuf text[3];
    uint64_t len[3] = {0, 0, 0};
    bool set[3] = {false, false, false};
    DevBufList bufs() { return {&text[0], &text[1], &text[2]}; }
    void forget() { for (bool &s : set) s = false; }
};

struct pgrc_mem_ctx {
    pgrc_match_ctx *base = nullptr;   // owns the packed source, its reverse complement, the seed index and the error text
    MemSource src;
    MemDest dst;
    MemEvents evs;
    MemRuns runs;
    MemReplay rp;
    PhaseEvents<5> ev;                // phase timing of a match (created on first use)
    pgrc_mem_counters ctr{};
    PmBufs pm;
    PmResident res;
    // every device buffer of the context's own parts (the base context frees its own)
    DevBufList bufs() {
        DevBufList all;
        for (const DevBufList &part : {dst.bufs(), evs.bufs(), runs.bufs(), rp.bufs(), pm.bufs(), res.bufs()}) all.insert(all.end(), part.begin(), part.end());
        return all;
    }
    // a new source, or a source that was refused: nothing of the old one stays matched, mapped or resident
    void forget_source() {
        src.have = false;
        dst.ready = false;
        res.forget();
    }
};

// a refusal worded by mem.hip or pgmap.hip itself
static inline int mem_fail(pgrc_mem_ctx *m, int code, const std::string &text) {
    m->base->err = text;
    return code;
}

