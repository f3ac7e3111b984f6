// rlistord.hip -- the four entry points of include/pgrc_readslist_ord.h, the order-preserving mode of the reads list (DESIGN.md
// 4.20).  Their code is rlist.hip's, behind the hooks of rlistctx.h; this file gives them their exported names and is linked
// into libpgrc_rlist_ord.so alone, beside the product's objects, as verify.hip is into libpgrc_verify.so.
#include "pgrc_readslist_ord.h"
#include "rlistctx.h"

extern "C" {

int pgrc_rlist_export_original_order(pgrc_rlist *list, pgrc_match_ctx *matcher, const pgrc_rlist_export_org_args *args) {
    return pgrc_rl_export_original_order(list, matcher, args);
}

int pgrc_rlist_archive_encode_ord(pgrc_rlist *list, int32_t fast_level, pgrc_rlist_archive *out) { return pgrc_rl_archive_encode_ord(list, fast_level, out); }

int pgrc_rlist_positions(const pgrc_rlist_pairpos_args *args, pgrc_rlist_positions_out *out) { return pgrc_rl_positions(args, out); }

void pgrc_rlist_positions_free(pgrc_rlist_positions_out *out) { pgrc_rl_positions_free(out); }

}   // extern "C"
