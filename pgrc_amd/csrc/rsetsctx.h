// rsetsctx.h -- the divided read sets on the device (include/pgrc_readsets.h, readsets.hip) and what readsets.hip uses of
// the contexts at both ends of its edits: the divider (divide.hip), the overlap search (pgovl.hip), the matcher (api.hip).
// The read sets are a stage: stagectx.h's PgrcStage (through decctx.h, which rlistctx.h needs on top of this header).
#pragma once

#include "decctx.h"
#include "pgrc_readsets.h"

// one PackedConstantLengthReadsSet and its VectorMapping: n rows of rb bytes in `rows` (room for cap_rows), n original indexes
// and the guard in `map` (LQ and N; the HQ set keeps none)
struct RsSet {
    DevBuf rows, map;
    uint64_t n = 0, cap_rows = 0, cap_map = 0;
    uint32_t symbols = 0, rb = 0;
    bool disposed = false;
};

struct pgrc_rsets : PgrcStage {        // (the stream, the staging buffers, the error string)
    pgrc_rsets_params prm{};
    RsSet set[3];
    uint64_t A = 0;                     // records appended; readsTotalCount once finished
    bool finished = false;
    uint64_t hq_gen = 0;                // counts the edits of the HQ set
    // the overlap run pgrc_rsets_move_by_overlap accepts: the context, its run's serial, the HQ set's generation at that run
    const void *ovl_ctx = nullptr;
    uint64_t ovl_serial = 0, ovl_gen = 0;
    // scratch of the edits (grow-only): the class bytes, three counts per original index, the flags, per-row counts of a
    // removal, descriptors, scan folds, the words of the checks
    DevBuf cls, cnt[3], flags, desc[2], fold, words, stage_idx;
    PhaseEvents<4> ev;
    bool have_timing = false;
    pgrc_rsets_timing tm{};
};

// divide.hip: the sets of the divider's last run where they lie on its device (valid until its next run)
struct PgrcDividerLast {
    bool valid;
    int device;
    pgrc_divide_params prm;
    uint64_t n_records, cnt[3];
    uint32_t symbols[3], rb[3];
    const uint8_t *d_rows[3];
    const uint32_t *d_idx[2];
};
void pgrc_divider_last_device(const pgrc_divider *d, PgrcDividerLast *out);
// divide.hip: the symbol rows of the divider's last run where they lie (n_records rows of read_len bytes in record order, the
// records of a pair of files interleaved; 16 spare bytes behind them; valid until its next run; NULL after a failed run)
void pgrc_divider_last_reads_device(const pgrc_divider *d, const uint8_t **d_reads, uint64_t *n_records);

// pgovl.hip
// pgrc_ovl_run; rows_on_device: in->packed_rows is memory of the context's device, complete when the call is made
int pgovl_run_rows(pgrc_ovl_ctx *o, const pgrc_ovl_input *in, pgrc_ovl_result *out, bool rows_on_device);
// the flags of pgrc_ovl_both_sides left on the device (R bytes, complete on return)
int pgovl_both_sides_device(pgrc_ovl_ctx *o, const uint8_t **d_flags, uint64_t *R);
int pgovl_device(const pgrc_ovl_ctx *o);
uint64_t pgovl_run_serial(const pgrc_ovl_ctx *o);      // counts the context's runs; 0 = no run of it stands

// api.hip: pgrc_match_append_reads_packed with the rows in memory of the context's device
int pgrc_append_rows_device(pgrc_match_ctx *c, const uint8_t *d_packed, uint64_t count, int32_t symbols);
