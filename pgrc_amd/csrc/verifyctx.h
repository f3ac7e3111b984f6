// verifyctx.h -- the verifier of include/pgrc_verify.h (verify.hip) and what selftest.hip reaches of it.  The handle is a
// stage: stagectx.h's PgrcStage (through rsetsctx.h, which also declares what verify.hip uses of the divider).  DESIGN.md 4.23.
#pragma once

#include "pgrc_verify.h"
#include "rsetsctx.h"

#define VF_CHUNK_BYTES (64ull << 20)    // IN_ORDER: rebuilt rows of one chunk
#define VF_PAD 16                       // bytes behind every buffer of rows: the aligned 8-byte loads of a row's last bytes stay inside
#define VF_SALTS 3

// one side's items where they lie: row r of file f at p[f] + r * stride[f]
struct VfSide {
    const uint8_t *p[2];
    uint64_t stride[2];
    uint64_t n;                         // items
};

struct VfCounts {                       // the counters of one salt, as the device leaves them
    unsigned long long matched, undecided, s_unmatched, d_unmatched, first_s, first_d;
};

struct pgrc_verify : PgrcStage {
    pgrc_decode_ctx *job = nullptr;
    int32_t kind = 0;
    uint32_t F = 1, L = 0;
    uint64_t key_mask = ~0ull;          // tests: the keys of this handle are cut to their low bits (pgrc_vf_mask_next_begin)
    uint64_t n_src[2] = {0, 0}, n_dec[2] = {0, 0};
    bool finished = false;
    pgrc_divider *divider = nullptr;    // add_fastq: made on first use
    // IN_ORDER: two chunks of source rows and of rebuilt rows, used in turn; ev_cmp[k]: the compare of chunk k has read them
    DevBuf src_chunk[2], dec_chunk[2], counters;
    hipEvent_t ev_cmp0[2]{}, ev_cmp[2]{};
    bool cmp_pending[2] = {false, false};
    int turn = 0;
    // MULTISET: the source rows per file (grow-only, contents kept), the rebuilt rows per file, keys and values in turn, the
    // run numbers, the head positions, the scan of the side bit, the sort's scratch
    DevBuf store[2], dec_rows[2], key[2], val[2], run_no, head_pos, side_cum, sort_scratch;
    PhaseEvents<5> ev;
    std::chrono::steady_clock::time_point t_begin;
    pgrc_verify_timing tm{};
};

// verify.hip, for selftest.hip: a verifier without a job (item = one row of `item_bytes` bytes), closed with pgrc_verify_end
int pgrc_vf_open(int32_t device, uint32_t item_bytes, pgrc_verify **out);
// phases 2-4 on keys given by the caller: v->key[0] holds the n_s + n_d keys, source first; the sides lie in device memory
int pgrc_vf_match_keys(pgrc_verify *v, const VfSide &s, const VfSide &d, VfCounts *out);
// the next pgrc_verify_begin of the process cuts its keys to the low `bits` bits (0 or 64 and above: no cut); taken at that begin
void pgrc_vf_mask_next_begin(uint32_t bits);
// grow-only buffers of the handle for a caller that fills them itself (PGRC_E_ALLOC names the bytes)
int pgrc_vf_key_buffers(pgrc_verify *v, uint64_t n);
// verify.hip, for readstext.hip: source text of any format (PGRC_READS_*, pgrc_reads.h) through the divider; `who` names the
// entry point in the error texts ("add_fastq", "add_text")
int pgrc_vf_add_text(pgrc_verify *v, const char *who, int32_t format, const char *text, uint64_t bytes, const char *pair_text, uint64_t pair_bytes,
                     int32_t final_piece, uint64_t *consumed, uint64_t *pair_consumed, uint64_t *n_records);
