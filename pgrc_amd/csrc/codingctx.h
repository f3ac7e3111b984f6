// codingctx.h -- the states of the three list codings of include/pgrc_decode.h: the pair positions (pairpos.hip), the pair
// order (pairorder.hip) and the archive form of a list's mismatch streams (listarchive.hip).  Each holds its grow-only device
// buffers, the events of its phases and the timing of its last call, and nothing else: a coder runs on any stage handle
// (stagectx.h) beside the state it is given.  The decode context (decctx.h) holds one of each behind the exported entry
// points; the reads list (rlistctx.h) holds one of each for the encode halves it runs on lists that lie on the device.  The
// pair order's decoder has a state of its own, which only the decode context holds.
#pragma once

#include "pgrc_decode.h"
#include "stagectx.h"

// the pair-position coding: the uploaded input, the sort's records (and values, W = 8) in turn, per-rank and per-far-pair
// arrays, the device-side output, scan scratch; sort: the (pooled) scratch of radix.hip's sort
struct PgrcPairPos {
    DevBuf in, rec[2], val[2], rank, far, out, bsum;
    DevBuf sort;
    PhaseEvents<6> ev;
    bool have_timing = false;
    pgrc_pairpos_timing tm{};
    DevBufList bufs() { return {&in, &rec[0], &rec[1], &val[0], &val[1], &rank, &far, &out, &bsum}; }
    void release() { dec_free_all(bufs()); pgrc_buf_free(sort); ev.release(); }
};

// the pair-order coding: the joined orgIdx, rev, per-entry and per-pair arrays, the device-side streams, scan scratch and the
// two error words
struct PgrcPairOrder {
    DevBuf in, rev, ent, pair, out, bsum;
    PhaseEvents<11> ev;
    bool have_timing = false;
    pgrc_pairorder_timing tm{};
    DevBufList bufs() { return {&in, &rev, &ent, &pair, &out, &bsum}; }
    void release() { dec_free_all(bufs()); ev.release(); }
};

// the pair-order decoder: the uploaded streams, the flag scans and every pair's offset, the landed pairs (COMPLETE: gathered
// from there), the landing's bitmap and the check's, scan scratch with the error, count and statistics words, the result of
// pgrc_pairorder_decode before it goes down
struct PgrcPairOrderDec {
    DevBuf in, pair, land, marks, bsum, out;
    PhaseEvents<7> ev;
    bool have_timing = false;
    pgrc_pairorder_decode_timing tm{};
    DevBufList bufs() { return {&in, &pair, &land, &marks, &bsum, &out}; }
    void release() { dec_free_all(bufs()); ev.release(); }
};

// the archive form of the mismatch streams: the uploaded streams, the flag scan, the counts (decode), the mismatch-list starts
// (encode), the count matrix and its scan scratch, the per-count words, the device-side block
struct PgrcListArchive {
    DevBuf in, inc, cnt, mcum, mat, fold, small, out;
    PhaseEvents<5> ev;
    bool have_timing = false;
    pgrc_list_archive_timing tm{};
    DevBufList bufs() { return {&in, &inc, &cnt, &mcum, &mat, &fold, &small, &out}; }
    void release() { dec_free_all(bufs()); ev.release(); }
};
