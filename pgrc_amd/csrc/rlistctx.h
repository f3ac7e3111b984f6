// rlistctx.h -- a pseudogenome's reads list on the device (include/pgrc_readslist.h, rlist.hip) and what rlist.hip uses of the
// contexts that fill and consume it: the assembly (pgasm.hip), the read sets (readsets.hip), the matcher's export
// (export.hip), the archive form (listarchive.hip), the pair order (pairorder.hip) and the pair positions (pairpos.hip).
// Every hook is a C++ function: exports.map keeps it out of the library's dynamic symbols.  The list is a stage handle
// (stagectx.h) with the states of the three codings it runs (codingctx.h) and its own buffers on top; the coders' hooks take
// the stage and the state.
#pragma once

#include "pgrc_assemble.h"
#include "pgrc_readslist.h"
#include "pgrc_readslist_ord.h"
#include "codingctx.h"
#include "rsetsctx.h"

// off (u16), org_idx (u32) and the optional streams of one list; every buffer is exactly the list's (grow-only scratch lies
// in the object, not here), so a new content is made beside the old one and swapped in
struct RlBufs {
    DevBuf off, org, rc, cnt, sym, roff;
    uint64_t n = 0, nmis = 0, last_pos = 0;
    uint32_t off_width = 1;             // bytes of an offset on output and of an element of roff
    bool has_rc = false, has_mis = false;
};

struct pgrc_rlist : PgrcStage {
    PgrcListArchive la;                 // the encode halves of the three codings run on this stage with these states
    PgrcPairOrder po;
    PgrcPairPos pp;
    RlBufs cur;
    // scratch (grow-only): a mapping / the reads' original indexes, the words of the checks, the device side of the archive
    // block, the joined lists, positions and their scan, the class bytes
    DevBuf map, words, block, join, pos, scan, cls;
    PhaseEvents<4> ev;                  // the phases of a call
    hipEvent_t ev_x[2]{};               // the hand-overs between this stream and a matcher's
    bool have_timing = false;
    pgrc_rlist_timing tm{};
};

// pgasm.hip: the reads list of the context's last successful run where it lies (valid until its next run)
struct PgasmLastList {
    bool valid, mapped;                 // mapped: that run applied a host mapping (in->index_mapping)
    int device;
    uint64_t n, pg_len;
    uint32_t read_len;
    const uint32_t *d_org;
    const uint16_t *d_off;
};
void pgasm_last_list(const pgrc_asm_ctx *a, PgasmLastList *out);

// pgovl.hip: pgrc_ovl_assemble; list_stays: without the copy of the reads list to the host (res->org_idx, res->off stay NULL)
int pgovl_assemble(pgrc_ovl_ctx *o, pgrc_asm_ctx *a, const uint32_t *index_mapping, pgrc_asm_result *res, bool list_stays);

// readsets.hip: the mapping of set `which` on the device, *entries indexes in front of the guard (HQ: see there)
int pgrc_rsets_mapping_device(pgrc_rsets *s, int32_t which, const uint32_t **d_map, uint64_t *entries);

// export.hip: exportMatchesInPgOrder with the old list and the reads' original indexes (NULL: as args say) in memory of the
// matcher's device, complete when the call is made; the merged list stays in pooled buffers of the matcher until the release
struct PgrcExportListSrc {
    uint64_t count;
    const uint16_t *d_off;
    const uint32_t *d_org;
    const uint8_t *d_rc;                // NULL = all forward
    const uint32_t *d_read_org;
};
struct PgrcExportResident {
    uint64_t n_entries, n_mismatches, last_pos;
    uint32_t mis_off_width;             // bytes of an element of d_rev_off; d_off is 16 bits wide whatever the mode
    const uint16_t *d_off;
    const uint32_t *d_org;
    const uint8_t *d_rc, *d_cnt, *d_sym;
    const void *d_rev_off;
    void *keep;
};
int pgrc_export_pg_order_resident(pgrc_match_ctx *c, const pgrc_export_pg_order_args *x, const PgrcExportListSrc *src, PgrcExportResident *res);
// exportMatchesInOriginalOrder likewise: the reads' original indexes in memory of the matcher's device (NULL: x->read_org_idx
// goes up), the entry list left in pooled buffers of the matcher until the release; last_pos is 0 as the host call's
int pgrc_export_original_order_resident(pgrc_match_ctx *c, const pgrc_export_original_order_args *x, const uint32_t *d_read_org, PgrcExportResident *res);
void pgrc_export_resident_release(PgrcExportResident *res);

// listarchive.hip: pgrc_list_archive_encode's device side on streams that lie on the device; the block is written at d_block
// (pgrc_la_device_bytes), complete on return.  A host copy of its first `down` bytes with room for pgrc_la_host_bytes is
// described by pgrc_la_describe_resident, which also writes the props behind the streams.
struct PgrcLaResident {
    uint64_t down;
    uint32_t n_nonzero, limit;
    uint8_t order[5];
    uint64_t h_small[768];
};
uint64_t pgrc_la_device_bytes(uint64_t n, uint64_t m);
uint64_t pgrc_la_host_bytes(uint64_t n, uint64_t m);
int pgrc_la_encode_resident(PgrcStage *s, PgrcListArchive &st, const uint8_t *d_cnt, const uint8_t *d_sym, const uint8_t *d_off, uint64_t n, uint64_t m, bool fast,
                            uint8_t *d_block, PgrcLaResident *res);
void pgrc_la_describe_resident(pgrc_list_archive_streams *out, uint8_t *blk, uint64_t n, uint64_t m, bool fast, const PgrcLaResident *res);

// pairorder.hip: pgrc_pairorder_encode on the joined array in memory of the stage's device
int pgrc_pairorder_encode_joined(PgrcStage *s, PgrcPairOrder &st, const uint32_t *d_joined, uint64_t T, int32_t form, pgrc_pairorder_streams *out);
// pairpos.hip: pgrc_pairpos_encode on positions in memory of the stage's device, read where they lie
int pgrc_pairpos_encode_device(PgrcStage *s, PgrcPairPos &st, const uint64_t *d_org_idx_to_pos, uint64_t n_total, uint32_t pos_width, pgrc_pairpos_streams *out);

// rlist.hip: the order-preserving mode's calls, exported under the names of pgrc_readslist_ord.h by rlistord.hip
int pgrc_rl_export_original_order(pgrc_rlist *list, pgrc_match_ctx *matcher, const pgrc_rlist_export_org_args *args);
int pgrc_rl_archive_encode_ord(pgrc_rlist *list, int32_t fast_level, pgrc_rlist_archive *out);
int pgrc_rl_positions(const pgrc_rlist_pairpos_args *args, pgrc_rlist_positions_out *out);
void pgrc_rl_positions_free(pgrc_rlist_positions_out *out);
