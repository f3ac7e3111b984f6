// memctx.h -- the context behind include/pgrc_mem.h, shared by the matcher (mem.hip) and the mapping of its matches (pgmap.hip).
#pragma once

#include <string>

#include "ctx.h"
#include "pgrc_mem.h"

struct pgrc_mem_ctx {
    pgrc_match_ctx *base = nullptr;   // owns the packed source, its reverse complement and the seed index
    uint32_t L = 0;
    int K = 0, k1 = 0, k2 = 0, LK2 = 0, KLK24 = 0;
    const char *src = nullptr;        // borrowed host text; null after pgrc_mem_set_src_device (the packed words are all there is)
    uint64_t N = 0;
    bool have_src = false;
    DevBuf d_dest, d_nmap, d_stage, d_flag, d_cursor, d_evk[2], d_evv[2], d_tmp, d_scan, d_orun, d_oflag;
    DevBuf d_skey[2], d_sidx[2], d_first, d_runid, d_rstart, d_rend;   // events by (diagonal, window): sort ping-pong, runs
    DevBuf d_rdend, d_outc, d_ebstart, d_ebin, d_ebout, d_ebinc, d_small, d_match;   // the replay: per run, per event, per event block
    PhaseEvents<5> ev;                // phase timing (created on first use)
    pgrc_mem_counters ctr{};
    std::string err;

    // the destination of the last successful pgrc_mem_match_texts, as pgrc_mem_mark_and_remove maps it (pgmap.hip): packed in
    // pg2[0] (dest_is_src) or in d_dest / d_nmap, which then hold the text as it was handed over (the reverse complement when
    // rev_compl)
    bool map_ready = false, map_dest_is_src = false, map_rev_compl = false, map_has_n = false;
    uint64_t map_n2 = 0;
    DevBuf pm_in, pm_f[3], pm_key[2], pm_idx[2], pm_flag, pm_slot, pm_u[4], pm_pmax, pm_jump[2], pm_kept, pm_m[3], pm_dp, pm_len,
        pm_nb, pm_cum, pm_nbpos, pm_mp, pm_off, pm_lens, pm_out, pm_fold, pm_small;
    PhaseEvents<5> pm_ev;             // phases of the mapping (created on first use)
    float pm_ms[5] = {0, 0, 0, 0, 0}; // normalise + sort, path, streams, text, download
    // the mapped texts that pgrc_mem_mark_and_remove_resident left in HBM, slot 0 HQ, 1 LQ, 2 N: what pgrc_mem_encode_mapped
    // codes as one text (pgrc_mem_set_src_ascii forgets them)
    DevBuf pm_res[3];
    uint64_t res_len[3] = {0, 0, 0};
    bool res_set[3] = {false, false, false};
};

// pgmap.hip: the mapping's device buffers and events (pgrc_mem_destroy gives them back)
void pgrc_pgmap_release(pgrc_mem_ctx *m);
