// dualkern.h -- the dual kernel of mode c: ONE query per read over both strands' indexes (included by copmem.hip).
//
// Reference behaviour restated (not translated): CopMEMMatcher::processApproxMatchQueryTight, matching/copmem/
// CopMEMMatcher.cpp:483-566, run by CopMEMReadsApproxMatcher::executeMatching (matching/ReadsMatchers.cpp:421-451) once on the
// text and once on its reverse complement (DefaultReadsMatcher::matchConstantLengthReads, :162-172).
//
// A two-pass run (min_mismatches == 0) as ONE query per read over both strands' indexes.  A read window hashes to the same
// bucket number in both tables, so every seed probes the forward and the RC head together (the pair table puts them into one
// 128-byte line: one request); the forward bucket's entries are judged first, then the RC bucket's.  Each strand is a query
// of its own whose limit is additionally capped by what the other strand has found -- forward by the RC count (a forward
// alignment only matters if it is at least as good), RC by the forward count - 1 (it must be strictly better) -- and each
// stops by the early-stop rule against its capped limit.  Why the result is the reference's (all forward seeds, then all RC
// seeds): a query under ANY sequence of limits that never falls below the smallest count m_min among its candidates accepts
// the FIRST candidate with m_min and nothing after it, which is the reference's final alignment; the caps never fall below
// the counts that still matter.  All of it presupposes that no run would have cut a bucket by the falses budget: U bounds the
// falses of any run over the candidates seen so far (1 for a candidate whose head count -- or already its fingerprint --
// exceeds the starting limit or whose tail is clean, else 2); U > budget when a bucket of more than 4 entries is opened (a
// bucket of at most 4 is the same bucket whatever the falses count: CopMEMMatcher.cpp:510-514) -> the lane does that read
// again in the reference's order, right here (F_SEQ: the real forward query with its falses count and bucket truncation,
// then the real RC query from its result) -- hidden behind the other lanes.  oracle/pgrc_oracle.c restates the scheme
// (pgrc_or_match_copmem_dual); tests/test_early_stop_rule.py expects it to equal the reference's two passes on every input.
//
// Round 5: the per-read state machine on a register diet, so that SIX waves per SIMD are resident (80 registers; round 4: 96
// and five waves).  What went: the shifting copy of the read (10 registers at L = 150: a seed's window is now cut out of the
// read's LDS copy -- three ds_read_b32 and two alignbits -- and nothing is shifted when a lane moves to its next seed); the
// per-read counters, which now share five registers (`sr`, `cc`, `uu`, `ll`, `jn` below: every field is read with one v_bfe);
// the speculative first attempt, the redo rule and the hand-out direction as run-time parameters (measured in round 4, kept
// in DESIGN.md's appendix of dead ends).  16 staged reads per wave instead of 32 keep a block at 26.1 KB of LDS: six blocks
// per CU.
//
// Round skip (a.skip; PGRC_ROUND_SKIP=0 turns it off).  Only the seeds of a round can make a round clean; the other seeds of
// a round period matter only if they yield an acceptance.  So when a round ends and a strand is still active, the lane jumps
// to the next round's first seed (F_SKIP; the first passed-over seed and both strands' clean rounds are kept in `fl`) and
// probes round seeds only: every bucket whole (no truncation by the budget, no F_REDO), U left alone, nothing accepted.  A
// candidate of an active strand s with a count <= eff(s), or the end of the seeds, REWINDS the lane: back to the first
// passed-over seed with the clean rounds of that moment and no dirty round, from where it goes on in seed order as without
// the rule (and may skip again at the next round end).  A strand whose clean rounds exceed eff(s) in skip mode stops, as
// always.  Why the result is the same: that strand stops only after eff(s) + 1 clean rounds without a candidate <= eff(s);
// by the early-stop argument (copmem.hip, "Early stop") no alignment with <= eff(s) mismatches exists anywhere in the text,
// so no passed-over seed could have been accepted, whatever the falses budget would have cut.  eff(s) only falls, so such a
// stop still holds after a later rewind of the other strand.  Everything else is replayed in seed order, so ties, limits
// and U (an upper bound of the falses of the reference's run: skip mode adds nothing to it) come out as before.  F_SEQ never
// skips.  tests/roundskip_model.py restates the rule; tests/test_round_skip_rule.py holds it to the reference's order.
//
// The refill.  A wave reserves a.chunk reads at a time from one work counter, stages SW of them in LDS (lanes 0 .. SW - 1: a
// full line per row and side item) and hands them to the lanes that have finished their read; a wave that was told once that
// the counter is past n never asks it again (`dry`: otherwise every iteration of the drain in which a lane finishes is a
// round trip of the whole wave to the one word all waves share -- a fifth of C2's kernel).  The stage's loads are six to
// eight dependent round trips in front of the iteration's gathers (the register cap lets the compiler issue them two at a
// time only).  Bringing them down to one (all 64 lanes, straight into LDS) and hiding that one behind the gathers (the stage
// decided an iteration ahead) was built and measured: nothing at C3 beyond the run-to-run spread -- a waiting wave is
// covered by the five others of its SIMD -- and a loss at -M 3; in registers it spills.  Not kept: DESIGN.md appendix A,
// profiles/stage_ahead_ab.txt, profiles/stage_ahead_kernel_resources.txt.  tests/test_gpu_dual_staging.py holds the refill
// to the oracle at chunk and stage boundaries.
//
// The entry walk.  A load brings a lane up to two entries of a bucket -- a head holds entry 0 and, of a two-entry bucket,
// entry 1; a fetch from ent[] brings a 16-byte pair -- and the lane goes over both in the iteration that brought them: the
// position test and the fingerprint reject an entry within a few instructions, without a load, and the first entry they
// let through goes down the chain (verify cache, then the judge or M_VERIFY).  Only an entry that waits behind one that went
// to M_VERIFY still costs an iteration of its own (`pend_e`).  Before, every entry took an iteration: 312 M of C3's 1 488 M
// lane-iterations per launch moved a lane to an entry it already held (profiles/entry_walk_mix.txt).  The entries, their
// order and the limit each one meets are the same, and so are all counters.  Wider fetches (four or six entries) were
// measured and are not kept.  The refill makes its LDS addresses from a copy of the thread index that
// the compiler cannot see through, so that they are not kept in registers through every iteration: the C3 instance is at 70
// registers (77 before).  tests/test_gpu_dual_entry_walk.py holds the walk to the oracle and to the parent kernel's counters
// on planted repeat families.
//
// The packed result (a.pack; PGRC_DUAL_PACK=0 turns it off).  A lane that finishes a matched read stored its position, strand
// and count to three arrays; lanes finish at different times, so each was a partial-line write of its own: 1.6 * 10^8 write
// requests and 7.1 GB per launch at C3 for 0.9 GB of results (profiles/packed_result_pmc.txt).  Now it is ONE 8-byte store to
// pos[]: position | count << 40 | strand << 48 | 1 << 62 (ctx.h RES_PACK_*; positions stay below 2^40: api.hip pgrc_pg_alloc).
// Bit 62 set and bit 63 clear is neither a plain position nor PGRC_NOT_MATCHED_POS, so k_unpack_results (results.hip), queued
// right behind the kernel over the same reads, knows the words this launch wrote, stores their three values in full lines and
// touches no other read: one whose query found nothing keeps what it came with (a second-phase run), a read of the byte path
// is the N kernel's.  The kernel itself reads mism[] only in the refill, for reads it has not started, and pos[] / rc[] never, so
// no lane ever sees a packed word.  tests/test_gpu_dual_packed_result.py holds both forms to the oracle and to each other.
#pragma once

#include "ctx.h"
#include "matchdev.h"

struct DualArgs {
    const uint32_t *pg[2];        // packed text, forward and reverse complement
    uint64_t G;
    const uint32_t *reads;
    uint64_t n, stride;
    const uint8_t *nflag;         // reads with N: 1 = the byte path of the ordinary passes, 3 = taken here, its N positions in npos
    const uint32_t *npos;         // (ctx.h nread_npos; nullptr: every flagged read goes the byte path)
    const ulonglong2 *head[2];    // head of bucket h of strand x at head[x][head_slot(h, hsh)] (headfmt.h); the pair table: the two
    uint32_t hsh;                 // heads of a bucket number share a line (one line request and one translation for both gathers)
    const uint64_t *ent[2];
    uint64_t *pos;
    uint8_t *rc;
    uint8_t *mism;
    PgrcDualCounters *counters;   // (matchdev.h)
    unsigned long long *work;
    uint8_t *redo_flag;           // per read: 2 = done again in the reference's order (F_SEQ); introspection only
    uint32_t L, K, k1, k2, mask, kmax;
    uint32_t chunk;               // reads a wave reserves per visit to the work counter (pgrc_match_chunk)
    uint32_t skip;                // 1: the round skip (see above); 0: every seed up to the early stop (PGRC_ROUND_SKIP=0)
    uint32_t pack;                // 1: a finished read is ONE store, the packed word in pos[] (see above); 0: three stores (PGRC_DUAL_PACK=0)
};

// reads a wave stages in LDS per burst of full-line loads: 16 at six waves per SIMD (LDS for six blocks per CU), else 32
template <int WAVES> struct DualStage { static constexpr int SW = WAVES >= 6 ? 16 : 32; };

// 16-byte gathers with the non-temporal hint (global_load_dwordx4 ... nt): the same 128-byte line request, 11 % more of them per second
// on random lines (tools/ubench/gather_modes.hip, profiles/r05_ubench_gather_modes.txt)
typedef unsigned long long dk_v2u64 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ ulonglong2 dk_ld_nt(const ulonglong2 *p) {
    const dk_v2u64 v = __builtin_nontemporal_load(reinterpret_cast<const dk_v2u64 *>(p));
    return make_ulonglong2(v.x, v.y);
}

template <int NW, int KQ, bool POS64, int WAVES>
__global__ void __launch_bounds__(MATCH_TPB) __attribute__((amdgpu_waves_per_eu(WAVES)))
k_copmem_match_dual(const DualArgs a) {
    typedef typename std::conditional<POS64, uint64_t, uint32_t>::type pos_t;
    constexpr pos_t POS_NONE = (pos_t)~(pos_t)0;
    constexpr uint32_t EPOCH_BITS = POS64 ? 12u : 14u;   // the verify cache's tag: epoch | strand | (POS64: position bits 32..39)
    constexpr int SW = DualStage<WAVES>::SW;
    // window words a seed's hash looks at (K = 28: 56 bits = 2 words), and the read words they are cut from
    constexpr int NWIN = KQ ? (KQ * 8 + 31) / 32 : 4, NSRC = NWIN + 1;
    __shared__ uint32_t lut[PGRC_HASH_LUT_WORDS];
    __shared__ uint32_t fpm_tab[SM_MAX_SEEDS];
    __shared__ uint2 vcache[VC_SLOTS][MATCH_TPB];
    __shared__ uint32_t rd_lds[NW][MATCH_TPB];   // the read: its windows are cut from here, and it is what a verified text window is compared with
    __shared__ uint32_t stg[MATCH_TPB / 64][NW][SW];
    __shared__ uint8_t stg_c[MATCH_TPB / 64][SW], stg_f[MATCH_TPB / 64][SW];
    __shared__ uint32_t stg_n[MATCH_TPB / 64][SW];
    __shared__ ulonglong2 hdR_lds[MATCH_TPB];    // the RC head of a lane's current seed, waiting for the forward bucket to finish
    uint32_t wbeg = 0, wend = 0, wnext = 0;
    bool dry = false;                            // the work counter is past n: no chunk is left to reserve
    hash_lut_init(lut);
    const int H = ((int)a.L / 8) * 8;
    const uint32_t nseeds = (a.L - a.K) / a.k2 + 1;
    for (uint32_t t = threadIdx.x; t < nseeds && t < SM_MAX_SEEDS; t += blockDim.x)
        fpm_tab[t] = fp_head_mask(a.K, t * a.k2, (uint32_t)H);
#pragma unroll
    for (int k = 0; k < VC_SLOTS; k++) vcache[k][threadIdx.x] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    uint32_t n_search = 0, n_cand = 0, n_probe = 0, n_ent = 0, n_ver = 0, n_redo = 0, n_seed = 0;   // wave-uniform: SGPRs
    uint32_t n_skip = 0, n_rew = 0;
    const uint32_t budget = (a.L + 1u - a.K) / a.k2;
    const uint32_t rper = (a.K + a.k1 * a.k2 - 1u) / (a.k1 * a.k2) * a.k1;

    enum { M_PROBE = 0, M_ENTRY = 1, M_VERIFY = 2, M_NEED = 3, M_ADV = 4, M_DEAD = 5 };
    // F_SEQ: the falses bound ran out: the lane does this read again in the reference's order, right here (forward query
    // with its real falses count and bucket truncation, then -- F_SEQ1 -- the RC query from the forward result)
    // F_SKIP: round seeds only (the round skip); bits 11..30 of fl then hold the first passed-over seed (8 bits) and both
    // strands' clean rounds when the lane started skipping (6 bits each: a read has at most (L - K) / K + 2 < 16 rounds).
    // F_SKIPPED: the read has skipped (counted once).
    enum { F_ACT0 = 1, F_ACT1 = 2, F_FOUND0 = 4, F_FOUND1 = 8, F_DIRTY0 = 16, F_DIRTY1 = 32, F_REDO = 64, F_FWDEXACT = 128,
           F_SEQ = 256, F_SEQ1 = 512, F_SKIP = 1024, F_SKIPPED = 1u << 31 };
    // ---- the lane's read.  Five registers hold what round 4 kept in twenty:
    //   sr = si | rq << 8 | rcl0 << 16 | rcl1 << 24      seed index (< 240), seed inside the round period, clean rounds per strand
    //   cc = cur0 | cur1 << 8 | cin << 16 | L0 << 24     best count per strand, the read's count before the run, its starting limit
    //   uu = U0 | U1 << 16                               bound on the falses of any run, per strand (<= 2 x 13 x 240)
    //   ll = (lim0 + 1) | (lim1 + 1) << 9 | epoch << 18  own limit per strand (-1 once an exact alignment is accepted)
    //   jn = j | nb << 4 | x << 8 | has_pend << 9        entry index and size of the bucket being gone through, its strand
    uint32_t mode = M_NEED, idx = 0, fl = 0;
    uint32_t sr = 0, cc = 0, uu = 0, ll = 0, jn = 0;
    uint32_t npw = 0xFFFFFFFFu;   // the read's N positions, one per byte (0xFF = none): a read with 1-4 N's (hash_fp_window_n)
    uint32_t cnext = 0, cend = 0;
    pos_t best0 = POS_NONE, best1 = POS_NONE;
    pos_t lo = 0;
    uint32_t fp_read = 0;
    pos_t cand_p = 0;
    uint64_t pend_e = 0;
    constexpr int PWN = ((NW + 1 + 3) / 4) * 4;
    // entries a fetch brings and a lane walks over in one iteration (even).  Two: a 16-byte pair, as a head holds.  Four and six
    // (two and three pairs per fetch) were measured: entry fetches 167 M -> 133 M / 129 M per launch at C3, the kernel no faster
    // than with two (four) or as slow as without the walk (six), and six spills in the 64-bit-position instances
    // (profiles/entry_walk_ab.txt, profiles/entry_walk_kernel_resources.txt).
    constexpr int WALK = 2;
#define DK_SI() (sr & 0xFFu)
#define DK_RQ() ((sr >> 8) & 0xFFu)
#define DK_RCL(s) ((sr >> (16u + 8u * (s))) & 0xFFu)
#define DK_CUR(s) ((cc >> (8u * (s))) & 0xFFu)
#define DK_CIN() ((cc >> 16) & 0xFFu)
#define DK_L0() ((int)(cc >> 24))
#define DK_U(s) ((uu >> (16u * (s))) & 0xFFFFu)
#define DK_LIM(s) ((int)((ll >> (9u * (s))) & 0x1FFu) - 1)
#define DK_EPOCH() (ll >> 18)
#define DK_J() (jn & 15u)
#define DK_NB() ((jn >> 4) & 15u)
#define DK_X() ((jn >> 8) & 1u)
#define DK_PEND() ((jn >> 9) & 1u)

    // the limit a candidate of strand s is judged against: its own, capped by what the other strand has found
    auto eff = [&](uint32_t s) -> int {
        const int own = DK_LIM(s);
        if (fl & F_SEQ) return own;                                  // the reference's order: no coupling
        if (s == 0u) return (fl & F_FOUND1) ? min(own, (int)DK_CUR(1u)) : own;
        return (fl & F_FOUND0) ? min(own, (int)DK_CUR(0u) - 1) : own;
    };
    auto set_lim = [&](uint32_t s, int v) { ll = (ll & ~(0x1FFu << (9u * s))) | ((uint32_t)(v + 1) << (9u * s)); };
    auto set_cur = [&](uint32_t s, uint32_t v) { cc = (cc & ~(0xFFu << (8u * s))) | (v << (8u * s)); };
    // the end of skip mode: back to the first passed-over seed (inside its round period: k1), its clean rounds, no dirty round
    auto rewind = [&]() {
        sr = ((fl >> 11) & 0xFFu) | (a.k1 << 8) | (((fl >> 19) & 63u) << 16) | (((fl >> 25) & 63u) << 24);
        fl &= (uint32_t)(F_SKIPPED | (F_SKIP - 1)) & ~(uint32_t)(F_DIRTY0 | F_DIRTY1);
        jn &= ~(1u << 9);
    };

    for (;;) {
        // ---- refill (as in k_copmem_match_sm, staged)
        const unsigned long long need = __ballot(mode == M_NEED);
        if (need) {
            // (The refill is the rare path.  Its LDS addresses, lane masks and the cache-clearing constant are made here, from
            // a copy of the thread index the compiler cannot see through: otherwise it keeps them in registers through every
            // iteration -- seven registers of the C3 instance, which the entry walk needs.)
            uint32_t tq = threadIdx.x;
            __asm__ volatile("" : "+v"(tq));
            const uint32_t wv = tq >> 6, lane = tq & 63u;
            // (dry: the counter only grows, so a wave that was told "past n" once never asks again.  Without it every
            // iteration of the drain in which a lane finishes is one more round trip of the whole wave to the one word all
            // waves share -- up to 64 per wave: 1.3 ms of C2's 6.4 ms, profiles/stage_ahead_ab.txt.)
            if (cnext == cend && !dry) {
                unsigned long long base = 0;
                if (lane == 0) base = atomicAdd(a.work, (unsigned long long)a.chunk);
                base = __shfl(base, 0, 64);
                const uint32_t lo_ = (uint32_t)min((uint64_t)base, a.n), hi_ = (uint32_t)min((uint64_t)base + a.chunk, a.n);
                // the chunks are handed out from the END of the read set (each still walked upwards): PgRC's sum set ends with
                // the N set, whose reads rarely match exactly and probe five times the buckets of an average read -- taken
                // last they are what the last waves still work on when the others have run dry (profiles/r04_from_end_ab.txt)
                cnext = __builtin_amdgcn_readfirstlane((uint32_t)a.n - hi_);
                cend = __builtin_amdgcn_readfirstlane((uint32_t)a.n - lo_);
                dry = cnext == cend;
            }
            if (wnext == wend && cnext != cend) {
                const uint32_t nst = min((uint32_t)SW, cend - cnext);
                wbeg = wnext = cnext;
                wend = cnext = __builtin_amdgcn_readfirstlane(cnext + nst);
                if (lane < nst) {
#pragma unroll
                    for (int k = 0; k < NW; k++) stg[wv][k][lane] = a.reads[(uint64_t)k * a.stride + wbeg + lane];
                    stg_c[wv][lane] = a.mism[wbeg + lane];
                    stg_f[wv][lane] = a.nflag ? a.nflag[wbeg + lane] : (uint8_t)0;
                    stg_n[wv][lane] = a.npos ? a.npos[wbeg + lane] : 0xFFFFFFFFu;
                }
                __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            const uint32_t avail = wend - wnext;
            if (avail == 0) {
                if (mode == M_NEED) mode = M_DEAD;
            } else {
                const uint32_t rank = (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
                const uint32_t take = min((uint32_t)__popcll(need), avail);
                bool started = false;
                if (mode == M_NEED && rank < take) {
                    const uint32_t sj = wnext - wbeg + rank;
                    idx = wbeg + sj;
                    const uint32_t cin = stg_c[wv][sj];
                    const uint32_t nfl = stg_f[wv][sj];
                    if ((nfl == 0u || (nfl == 3u && a.npos)) && cin != 0u) {   // ReadsMatchers.cpp:430 with min_mismatches == 0
                        npw = nfl ? stg_n[wv][sj] : 0xFFFFFFFFu;
#pragma unroll
                        for (int k = 0; k < NW; k++) rd_lds[k][threadIdx.x] = stg[wv][k][sj];
                        const uint32_t L0 = (cin < a.kmax) ? cin - 1u : a.kmax;   // :488-489
                        cc = cin | (cin << 8) | (cin << 16) | (L0 << 24);
                        uint32_t epoch = (DK_EPOCH() + 1u) & ((1u << EPOCH_BITS) - 1u);
                        if (epoch == 0) {
#pragma unroll
                            for (int k = 0; k < VC_SLOTS; k++) vcache[k][tq] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
                            epoch = 1;
                        }
                        ll = (L0 + 1u) | ((L0 + 1u) << 9) | (epoch << 18);
                        best0 = best1 = POS_NONE;
                        uu = 0;
                        sr = 0;
                        jn = 0;
                        fl = F_ACT0 | F_ACT1;
                        started = true;
                        mode = M_PROBE;
                    }
                }
                wnext = __builtin_amdgcn_readfirstlane(wnext + take);
                n_search += (uint32_t)__popcll(__ballot(started));
            }
        }
        if (!__any(mode != M_DEAD)) break;

        const uint32_t m0 = mode;
        // ---- this iteration's loads
        // what the lane has at hand in the consume phase: the head of the bucket to open (e[0], e[1]), then the nh entries of
        // the bucket that it holds, in bucket order: e[0 .. nh) -- a head's one or two, what a fetch brought, or the entry kept
        // behind a verified one
        uint64_t e[WALK];
        uint32_t nh = 0;
        bool counted_ent = false;
        uint32_t nprobe_it = 0;
        bool n_redo_it = false, rew = false, skip_new = false;
        if (m0 == M_PROBE) {
            // the seed's window, cut out of the read's LDS copy: symbols s .. s + K - 1
            const uint32_t s = DK_SI() * a.k2, q = s >> 4, shb = (s & 15u) * 2u;
            uint32_t r[NSRC], w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < NSRC; k++) {
                const uint32_t row = min(q + (uint32_t)k, (uint32_t)NW - 1u);
                const uint32_t val = rd_lds[row][threadIdx.x];
                r[k] = (q + (uint32_t)k < (uint32_t)NW) ? val : 0u;
            }
#pragma unroll
            for (int k = 0; k < NWIN; k++) w[k] = funnel_r(r[k], r[k + 1], shb);
            uint32_t h;
            if (__any(npw != 0xFFFFFFFFu))                           // (wave-uniform: only waves that hold a read with N's take the patched hash)
                h = hash_fp_window_n<KQ>(w[0], w[1], w[2], w[3], a.K, lut, &fp_read, npw, s) & a.mask;
            else
                h = hash_fp_window<KQ>(w[0], w[1], w[2], w[3], a.K, lut, &fp_read) & a.mask;
            ulonglong2 hdF = make_ulonglong2(HEAD_EMPTY, HEAD_EMPTY), hr = hdF;
            // (the non-temporal hint: in-context A/B 63.4 -> 62.6 ms at C3; on the entry pairs it costs 1 %, on the text windows nothing)
            if (fl & F_ACT0) hdF = dk_ld_nt(&a.head[0][head_slot(h, a.hsh)]);
            if (fl & F_ACT1) hr = dk_ld_nt(&a.head[1][head_slot(h, a.hsh)]);
            hdR_lds[threadIdx.x] = hr;
            nprobe_it = ((fl & F_ACT0) ? 1u : 0u) + ((fl & F_ACT1) ? 1u : 0u);
            e[0] = (fl & F_ACT0) ? hdF.x : hr.x;                     // the seed's first bucket: the forward one if that strand is active
            e[1] = (fl & F_ACT0) ? hdF.y : hr.y;
        } else if (m0 == M_ENTRY) {
            if (DK_PEND()) {                                         // back from a verification: the entry kept behind the verified one
                e[0] = pend_e;
                nh = 1;
                jn &= ~(1u << 9);
            } else {
                // ONE fetch for the bucket's next entries, up to WALK of them from entry j on: 16-byte pairs as far as the
                // lane's bucket goes (as before, a lane reads at most one entry past its bucket's last)
                const uint32_t j = DK_J(), rem = DK_NB() - j;
                const uint64_t *src = (DK_X() ? a.ent[1] : a.ent[0]) + lo + j - 1;
#pragma unroll
                for (int k = 0; k < WALK; k += 2) {
                    if ((uint32_t)k < rem) {
                        const U64x2A8 q = *reinterpret_cast<const U64x2A8 *>(src + k);
                        e[k] = q.x;
                        e[k + 1] = q.y;
                    }
                }
                nh = min(rem, (uint32_t)WALK);
                counted_ent = true;
            }
        }
        // ---- consume.  What a lane does with this iteration's load is a short chain -- open a bucket -> look at an entry ->
        // judge a verified alignment -> what follows -- and its mode says at which link it enters.  The chain runs at most
        // twice: a forward bucket that ends in this iteration hands over to the RC head of the same seed.  Every link is ONE
        // piece of code.  (Up to round 5a the links were lambdas inlined at every call site -- three copies of the entry
        // link, four of the judge -- and every copy ran in every iteration for the few lanes that needed it: the kernel is
        // bound by the VALU instructions it issues, 95 % of the SIMD cycles, not by its memory requests.)
        uint32_t next = m0;
        bool bdone = false;           // the current strand's bucket is finished
        bool op = false, tp = false, jp = false;                     // pending: a bucket to open, an entry to look at, an alignment to judge
        uint32_t jmh = 0, jmt = 0;
        if (m0 == M_VERIFY) {
            const uint32_t x = DK_X();
            uint32_t pw[PWN];
            const uint32_t *src = (x ? a.pg[1] : a.pg[0]) + (cand_p >> 4);   // the text is padded: PWN words are always in bounds
#pragma unroll
            for (int k = 0; k < PWN; k += 4) {
                const u32x4 q = reinterpret_cast<const U32x4A4 *>(src + k)->v;
                pw[k] = q.x; pw[k + 1] = q.y; pw[k + 2] = q.z; pw[k + 3] = q.w;
            }
            const uint32_t b = ((uint32_t)cand_p & 15u) * 2u;
            uint32_t mh = 0, mt = 0;
            if (__any(npw != 0xFFFFFFFFu)) {                         // (wave-uniform) an N of the read equals no text symbol
#pragma unroll
                for (int k = 0; k < NW; k++) {
                    const uint32_t xr = funnel_r(pw[k], pw[k + 1], b) ^ rd_lds[k][threadIdx.x];
                    uint32_t d = (xr | (xr >> 1)) & 0x55555555u;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint32_t q = (npw >> (8 * i)) & 0xFFu;
                        d |= ((q >> 4) == (uint32_t)k) ? 1u << (2u * (q & 15u)) : 0u;   // (none = 0xFF: symbol 255 lies beyond every read)
                    }
                    mh += (uint32_t)__popc(d & sym_mask(k, 0, H));
                    mt += (uint32_t)__popc(d & sym_mask(k, H, (int)a.L));
                }
            } else {
                // all differing symbols in one running count; the tail (symbols H .. L - 1, fewer than 8: H = 8 * (L / 8), and
                // 16 (NW - 1) < L <= 16 NW) lies inside the read's LAST word
                uint32_t tot = 0, dl = 0;
#pragma unroll
                for (int k = 0; k < NW; k++) {
                    const uint32_t xr = funnel_r(pw[k], pw[k + 1], b) ^ rd_lds[k][threadIdx.x];
                    const uint32_t d = (xr | (xr >> 1)) & (k < NW - 1 ? 0x55555555u : sym_mask(NW - 1, 0, (int)a.L));
                    tot += (uint32_t)__popc(d);
                    if (k == NW - 1) dl = d;
                }
                mt = (uint32_t)__popc(dl & sym_mask(NW - 1, H, (int)a.L));
                mh = tot - mt;
            }
            const uint32_t epoch = DK_EPOCH();
            vcache[((uint32_t)cand_p * 0x9E3779B1u + x) >> (32 - VC_BITS)][threadIdx.x] =
                make_uint2((uint32_t)cand_p, POS64 ? (mh | (mt << 8) | ((uint32_t)((uint64_t)cand_p >> 32) << 11) | (x << 19) | (epoch << 20))
                                                   : (mh | (mt << 8) | (x << 16) | (epoch << 17)));
            jmh = mh;
            jmt = mt;
            jp = true;
        } else if (m0 == M_ENTRY) {
            tp = true;
        } else if (m0 == M_PROBE) {
            const uint32_t x = (fl & F_ACT0) ? 0u : 1u;
            jn = x << 8;
            op = true;
        }
#pragma nounroll
        for (int trip = 0; trip < 2; trip++) {
            if (op) {                                                // open the bucket of strand x for the current seed
                op = false;
                const uint32_t x = DK_X();
                const uint32_t cnt = head_count(make_ulonglong2(e[0], e[1]));
                if (!cnt) {
                    bdone = true;
                } else if (!(fl & (F_SEQ | F_SKIP)) && DK_U(x) > budget && cnt > PGRC_TRUNC_BUCKET) {
                    // some run could have cut THIS bucket to its first 4 entries by now (:510-514 -- all the budget ever does; a
                    // bucket of at most 4 is the same bucket whatever the falses count): not decidable this way -> the read again,
                    // in the reference's order.  (Skip mode opens every bucket whole: it accepts nothing, and what it proves
                    // absent is absent from the whole text.)
                    fl |= F_REDO;
                    next = M_NEED;
                } else {
                    uint32_t nb = cnt;
                    if ((fl & F_SEQ) && DK_U(x) > budget) nb = min(nb, PGRC_TRUNC_BUCKET);   // :510-514
                    if (DK_RQ() < a.k1 && (cnt >= PGRC_BUCKET_CAP || nb < cnt)) fl |= (x == 0u ? (uint32_t)F_DIRTY0 : (uint32_t)F_DIRTY1);
                    lo = (pos_t)(e[1] & W1_BASE_MASK);
                    jn = (nb << 4) | (x << 8);                       // j = 0
                    e[0] &= ENT_MASK;                                // what a head holds: entry 0, and entry 1 of a two-entry bucket
                    nh = cnt == 2u ? 2u : 1u;
                    tp = true;
                }
            }
            bool ap = false;                                         // an entry was examined: what follows it
            // the entries at hand (a head's one or two, what a fetch brought, the one kept behind a verified entry), in order:
            // a lane walks over those that lie outside the text for this seed or that the fingerprint rejects, up to the
            // first that passes; that one goes down the rest of the chain.  (A limit only changes through an acceptance, and
            // the walk ends in front of one: eff() is the same for every entry of a walk.  The loop stays in the wave's common
            // control flow, so the candidates are counted on the scalar side; it ends when no lane has an entry left.)
            bool pass = false;                                       // ... and its position is cand_p
            {
                const uint32_t x = DK_X(), si = DK_SI();
                const uint32_t s = si * a.k2;
                const int lim = eff(x);
                const uint32_t fpm = tp ? fpm_tab[si] : 0u;
                bool walk = tp;
                ap = tp;
                tp = false;
#pragma unroll
                for (int k = 0; k < WALK; k++) {
                    const bool live = walk && (uint32_t)k < nh;
                    if (!__any(live)) break;
                    bool inside = false;                             // :517-520
                    if (live) {
                        jn++;                                        // j++ (j <= 13: no carry into nb)
                        pos_t pk;
                        if (POS64) {
                            const uint64_t sp = e[k] >> PGRC_FP_BITS;
                            inside = (uint64_t)s <= sp && sp - s + a.L <= a.G;
                            pk = (pos_t)(sp - s);
                        } else {                                     // (G + 256 < 2^32: positions, and position + L, fit 32 bits)
                            const uint32_t sp = (uint32_t)(e[k] >> PGRC_FP_BITS);
                            inside = s <= sp && sp - s + a.L <= (uint32_t)a.G;
                            pk = (pos_t)(sp - s);
                        }
                        if (inside) {
                            const uint32_t xr = ((uint32_t)e[k] ^ fp_read) & ((1u << PGRC_FP_BITS) - 1u);
                            const int fpc = __popc((xr | (xr >> 1)) & fpm);   // a lower bound of the head count
                            if (fpc > lim) {
                                const uint32_t u = ((fl & F_SEQ) || fpc > DK_L0()) ? 1u : 2u;   // (sequential: a certain head reject)
                                if (!(fl & F_SKIP)) uu += u << (16u * x);
                            } else {
                                walk = false;
                                pass = true;
                                cand_p = pk;
                                if (k + 1 < WALK && (uint32_t)k + 1u < nh) {    // the entry behind it waits for the return from M_VERIFY
                                    pend_e = e[k + 1 < WALK ? k + 1 : k];
                                    jn |= 1u << 9;
                                }
                            }
                        }
                    }
                    n_cand += (uint32_t)__popcll(__ballot(inside));
                }
            }
            if (pass) {                                              // an entry inside the text that the fingerprint lets through
                const uint32_t x = DK_X();
                const uint32_t epoch = DK_EPOCH();
                const uint2 cv = vcache[((uint32_t)cand_p * 0x9E3779B1u + x) >> (32 - VC_BITS)][threadIdx.x];
                const bool hit = POS64 ? (cv.x == (uint32_t)cand_p && (cv.y >> 20) == epoch && ((cv.y >> 19) & 1u) == x &&
                                          ((cv.y >> 11) & 0xFFu) == (uint32_t)((uint64_t)cand_p >> 32))
                                       : (cv.x == (uint32_t)cand_p && (cv.y >> 17) == epoch && ((cv.y >> 16) & 1u) == x);
                if (hit) {
                    jmh = cv.y & 0xFFu;
                    jmt = (cv.y >> 8) & (POS64 ? 0x7u : 0xFFu);
                    jp = true;
                } else {
                    next = M_VERIFY;
                    ap = false;
                }
            }
            if (jp) {                                                // a verified alignment of the current strand (head count jmh, tail count jmt)
                jp = false;
                ap = true;
                const uint32_t x = DK_X();
                const int m = (int)(jmh + jmt);
                uint32_t u;
                if (fl & F_SEQ) {                                    // the real count of CopMEMMatcher.cpp:536-551
                    const int lm = eff(x);
                    u = ((int)jmh > lm) ? 1u : (m > lm) ? 2u : 0u;
                } else {
                    // what any run can count for this candidate: 1 if the head alone exceeds every limit a run can have, or if
                    // the tail is clean (then it is a head reject or an acceptance), else 2 (a tail reject is counted twice)
                    u = ((int)jmh > DK_L0() || jmt == 0u) ? 1u : 2u;
                }
                if (!(fl & F_SKIP)) uu += u << (16u * x);
                if (m <= eff(x) && (fl & F_SKIP)) {                  // acceptable, met in skip mode: the passed-over seeds in order
                    rewind();
                    rew = true;
                    next = M_PROBE;
                    ap = false;
                } else if (m <= eff(x)) {
                    set_cur(x, (uint32_t)m);
                    set_lim(x, m - 1);
                    if (x == 0u) { best0 = cand_p; fl |= F_FOUND0; }
                    else { best1 = cand_p; fl |= F_FOUND1; }
                    if (m == 0) {                                    // m <= min_mismatches: this strand's query returns
                        fl &= ~(x == 0u ? (uint32_t)F_ACT0 : (uint32_t)F_ACT1);
                        if (x == 0u) fl |= F_FWDEXACT;               // ... and the RC pass would skip the read
                    }
                }
            }
            if (ap) {                                                // what follows an examined entry
                if (fl & F_FWDEXACT) next = M_NEED;
                else if (!(fl & (DK_X() == 0u ? (uint32_t)F_ACT0 : (uint32_t)F_ACT1))) bdone = true;   // an exact RC alignment: that query is over
                else if (DK_J() < DK_NB()) next = M_ENTRY;
                else bdone = true;
            }
            // the forward bucket is done: the RC head of the same seed waits in LDS
            const bool chain = bdone && DK_X() == 0u && (fl & F_ACT1);
            if (!__any(chain)) break;
            if (chain) {
                bdone = false;
                jn = 1u << 8;
                const ulonglong2 hr = hdR_lds[threadIdx.x];
                e[0] = hr.x;
                e[1] = hr.y;
                op = true;
            }
        }
        if (bdone) next = M_ADV;
        if (next == M_ADV) {                                         // to the next seed
            const uint32_t rq = DK_RQ();
            uint32_t rcl0 = DK_RCL(0u), rcl1 = DK_RCL(1u);
            if (rq == a.k1 - 1u) {                                   // a round is behind this read
                rcl0 += (fl & F_DIRTY0) ? 0u : 1u;
                rcl1 += (fl & F_DIRTY1) ? 0u : 1u;
                fl &= ~(uint32_t)(F_DIRTY0 | F_DIRTY1);
            }
            uint32_t si = DK_SI() + 1u, rqn = rq + 1u == rper ? 0u : rq + 1u;
            jn &= ~(1u << 9);
            if ((fl & F_ACT0) && (int)rcl0 > eff(0u)) fl &= ~(uint32_t)F_ACT0;   // nothing acceptable is left on that strand
            if ((fl & F_ACT1) && (int)rcl1 > eff(1u)) fl &= ~(uint32_t)F_ACT1;
            if (rqn == a.k1 && a.skip && (fl & (F_ACT0 | F_ACT1)) && !(fl & F_SEQ)) {
                // a round is over and its period has seeds between it and the next round (rper > k1): pass over them
                const uint32_t nx = si + rper - a.k1;
                if (!(fl & F_SKIP) && nx < nseeds) {
                    skip_new = !(fl & F_SKIPPED);
                    fl |= F_SKIP | F_SKIPPED | (si << 11) | (rcl0 << 19) | (rcl1 << 25);
                }
                if (fl & F_SKIP) {
                    si = nx;
                    rqn = 0;
                }
            }
            sr = si | (rqn << 8) | (rcl0 << 16) | (rcl1 << 24);
            if ((fl & F_SKIP) && si >= nseeds && (fl & (F_ACT0 | F_ACT1))) {   // the seeds ran out in skip mode
                rewind();
                rew = true;
                si = DK_SI();
            }
            next = (si < nseeds && (fl & (F_ACT0 | F_ACT1))) ? M_PROBE : M_NEED;
        }
        // ---- the reference's order for a read whose falses bound ran out: restart it as a forward query, then an RC query
        if (next == M_NEED && m0 <= M_VERIFY && (((fl & F_REDO) != 0u) || ((fl & (F_SEQ | F_SEQ1 | F_FWDEXACT)) == F_SEQ))) {
            const bool second = (fl & F_SEQ) != 0u;                  // the forward query just ended: now the RC query
            const uint32_t cin = DK_CIN();
            if (!second) {
                set_lim(0u, DK_L0());
                set_cur(0u, cin);
                best0 = POS_NONE;
                uu &= 0xFFFF0000u;
                fl = F_SEQ | F_ACT0;
                n_redo_it = true;
                a.redo_flag[idx] = 2;
            } else {
                const uint32_t c1 = (fl & F_FOUND0) ? DK_CUR(0u) : cin;   // what the RC query has to beat (:488-489)
                set_lim(1u, (c1 < a.kmax) ? (int)c1 - 1 : (int)a.kmax);
                set_cur(1u, c1);
                best1 = POS_NONE;
                uu &= 0x0000FFFFu;
                fl = (fl & (F_FOUND0 | F_SEQ)) | F_SEQ1 | F_ACT1;
            }
            sr = 0;                                                  // first seed again; clean rounds of both strands reset (only the active one is read)
            jn &= ~(1u << 9);
            next = M_PROBE;
        }
        {
            const uint32_t seeds_it = (uint32_t)__popcll(__ballot(nprobe_it >= 1));
            n_seed += seeds_it;
            n_probe += seeds_it + (uint32_t)__popcll(__ballot(nprobe_it >= 2));
        }
        n_ent += (uint32_t)__popcll(__ballot(counted_ent));
        n_ver += (uint32_t)__popcll(__ballot(m0 == M_VERIFY));
        const bool fin = next == M_NEED && m0 <= M_VERIFY;
        if (fin) {
            // the read is finished: forward wins ties, RC must be strictly better (ReadsMatchers.cpp:437-447, both passes)
            const uint32_t cur0 = DK_CUR(0u), cur1 = DK_CUR(1u);
            const bool rcw = (fl & F_FOUND1) && !((fl & F_FOUND0) && cur0 <= cur1);
            if (rcw || (fl & F_FOUND0)) {
                const uint64_t p = rcw ? a.G - ((uint64_t)best1 + a.L) : (uint64_t)best0;
                const uint32_t m = rcw ? cur1 : cur0;
                if (a.pack) {                                        // (wave-uniform) one store; k_unpack_results takes it apart
                    a.pos[idx] = p | ((uint64_t)m << RES_PACK_MISM_SHIFT) | ((uint64_t)rcw << RES_PACK_RC_SHIFT) | RES_PACK_TAG;
                } else {
                    a.pos[idx] = p;
                    a.rc[idx] = (uint8_t)rcw;
                    a.mism[idx] = (uint8_t)m;
                }
            }
        }
        n_redo += (uint32_t)__popcll(__ballot(n_redo_it));
        n_skip += (uint32_t)__popcll(__ballot(skip_new));
        n_rew += (uint32_t)__popcll(__ballot(rew));
        mode = next;
    }
    if (a.counters && lane == 0) {
        atomicAdd(&a.counters->w.searched, (unsigned long long)n_search);
        atomicAdd(&a.counters->w.candidates, (unsigned long long)n_cand);
        atomicAdd(&a.counters->w.probes, (unsigned long long)n_probe);
        atomicAdd(&a.counters->w.entry_fetches, (unsigned long long)n_ent);
        atomicAdd(&a.counters->w.verifies, (unsigned long long)n_ver);
        atomicAdd(&a.counters->redo, (unsigned long long)n_redo);
        atomicAdd(&a.counters->seed_probes, (unsigned long long)n_seed);
        atomicAdd(&a.counters->skip_reads, (unsigned long long)n_skip);
        atomicAdd(&a.counters->rewinds, (unsigned long long)n_rew);
    }
#undef DK_SI
#undef DK_RQ
#undef DK_RCL
#undef DK_CUR
#undef DK_CIN
#undef DK_L0
#undef DK_U
#undef DK_LIM
#undef DK_EPOCH
#undef DK_J
#undef DK_NB
#undef DK_X
#undef DK_PEND
}
