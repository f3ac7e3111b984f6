// pgovl.hip -- the overlap search of the pseudogenome generator on the device: findOverlappingReads of
// GreedySwipingPackedOverlapGeneratorTemplate at one thread (GreedySwipingPackedOverlapPseudoGenomeGenerator.cpp:97-249) and
// getBothSidesOverlappedReads (AbstractOverlapPseudoGenomeGenerator.cpp:75-91); include/pgrc_overlap.h, DESIGN.md 4.15.
//
// The reference pops one suffix at a time from a queue of the symbol groups and walks a cursor through the sorted prefixes.
// Every decision of that loop is a function of ranks inside runs of equal strings and of the order of the five groups in front
// of a run, which folds over the runs with an associative operator (scanops.h ScoWeakOrder5).  A sweep i is
//   ranks      S (reads without a successor, sorted by the suffix from i - 1 on) lies in five groups by the symbol at i - 1, each
//              sorted by the suffix from i on.  Every suffix finds, by search in each group, how many suffixes there are below
//              it and how many equal it: the start of its run in the merged order, the groups' shares len_g of the run, its
//              rank inside its group's share.  A run's first suffix writes the run's transition (the dense ranks of len_g)
//   scan       the exclusive scan of the transitions, seeded with the symbol order: the groups' order in front of every run
//   place      the run comes out round robin over its groups in that order: a suffix's place is a sum over the five shares
//   pairing    a merged position finds its run's class in P (reads without a predecessor, sorted) by search, decides by the
//              closed form whether it takes the prefix at its own rank, the one before or the one after (a read that meets
//              its own prefix is held back one place), links, and applies the drop rule of :193
//   compaction the flags of S and P are scanned and both lists are written anew; the next groups are read off the new S
// The host reads two counters per sweep (what is left of S and of P) and ends when either is empty.
// PGRC_OVL_RULE_PARALLEL is findOverlappingReads of ParallelGreedySwipingPackedOverlapGeneratorTemplate instead: the
// groups' order starts anew with every block of three symbols (a reset bit in the same scan), nothing is dropped, the sweeps from
// L - 3 on pair whole blocks -- the first in the order of a merge by the rows that follow the reads, the other two regrouped
// by dropping a symbol.  The serial rule's kernels are the same templates with the switches off.
// Rows are unpacked once to a byte per symbol in rows of 8-byte words, so that eight symbols at any offset are two aligned
// loads, a shift and one compare.  Integer work bound by random row reads of the searches; no library kernel.
#include <chrono>
#include <cmath>
#include <vector>

#include "asmctx.h"
#include "devutil.h"
#include "pgrc_overlap.h"
#include "rsetsctx.h"

#define OV_TPB 256
#define OV_BLOCK_PREFIX 3u       // blockPrefixLength of the parallel generator
#define OV_CHUNK 8u             // symbols of one key of the order's sort: 3 bits each, 24 bits a key

// the words of `bad`, in the order the refusals are reported
enum { OV_BAD_ROW, OV_BAD_RANGE, OV_BAD_TWICE, OV_BAD_SORT, OV_BAD_PLACE, OV_BAD_WORDS };

struct pgrc_ovl_ctx : PgrcStage {
    DevBuf sort_scratch;
    DevBuf rows, sym, nx, ov, ovout, order, seen, eq, s[2], p[2], base, lens, rk, trans, merged, mk, keep, taken, offs, offp, gs, fold, words, rec[2], prev, flags;
    DevBuf rnk, lead, cnt;              // the parallel rule: the reads' dense ranks, the prefix maxima of a share, two counters
    PhaseEvents<4> ev;
    uint64_t R = 0;
    uint32_t L = 0, symbols = 0, rb = 0;
    bool have_run = false;
    uint64_t run_serial = 0;            // counts the runs (pgovl_run_serial: readsets.hip knows its own run by it)
    uint32_t rule = PGRC_OVL_RULE_SERIAL;
    pgrc_ovl_rule_info info{};
    pgrc_ovl_timing tm{};
    std::vector<float> sweep_ms;
};

static thread_local std::string g_ov_create_err;

static DevBufList ov_bufs(pgrc_ovl_ctx *o) {       // (sort_scratch is pooled)
    return {&o->rows, &o->sym, &o->nx, &o->ov, &o->ovout, &o->order, &o->seen, &o->eq, &o->s[0], &o->s[1], &o->p[0], &o->p[1], &o->base, &o->lens, &o->rk, &o->trans,
            &o->merged, &o->mk, &o->keep, &o->taken, &o->offs, &o->offp, &o->gs, &o->fold, &o->words, &o->rec[0], &o->rec[1], &o->prev, &o->flags, &o->rnk, &o->lead, &o->cnt};
}

// ------------------------------------------------------------------------------------------------ strings
// eight symbols of an unpacked row from `pos` on, the first one most significant.  A row is 8-byte aligned and ends with at
// least eight zero bytes after symbol L - 1, so the second word exists for every pos < L.
__device__ __forceinline__ uint64_t ov_ld8(const uint8_t *__restrict__ row, uint32_t pos) {
    const uint64_t *w = reinterpret_cast<const uint64_t *>(row) + (pos >> 3);
    const uint32_t s = (pos & 7u) * 8u;
    const uint64_t a = __builtin_bswap64(w[0]);
    if (!s) return a;
    return (a << s) | (__builtin_bswap64(w[1]) >> (64u - s));
}

// symbols [oa, oa + len) of row a against [ob, ob + len) of row b: -1, 0, 1 (oa + len, ob + len <= L)
__device__ __forceinline__ int ov_cmp(const uint8_t *__restrict__ a, uint32_t oa, const uint8_t *__restrict__ b, uint32_t ob, uint32_t len) {
    for (uint32_t k = 0; k < len; k += 8u) {
        uint64_t x = ov_ld8(a, oa + k), y = ov_ld8(b, ob + k);
        const uint32_t rem = len - k;
        if (rem < 8u) {
            const uint64_t mask = ~0ull << (8u * (8u - rem));
            x &= mask;
            y &= mask;
        }
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ kernels: the start
// one packed byte to its 4 or 3 symbols; ACGNT: a byte of 125 or more is no three digits, the digits after symbol L - 1 are zero
static __global__ void __launch_bounds__(OV_TPB) k_ov_unpack(const uint8_t *__restrict__ rows, uint64_t total, uint32_t rb, uint32_t symbols, uint32_t L, uint32_t stride,
                                                             uint8_t *__restrict__ sym, uint32_t *__restrict__ bad) {
    for (uint64_t g = (uint64_t)blockIdx.x * OV_TPB + threadIdx.x; g < total; g += (uint64_t)gridDim.x * OV_TPB) {
        const uint32_t v = rows[g], b = (uint32_t)(g % rb);
        uint8_t *out = sym + (g / rb) * stride;
        if (symbols == 4) {
            for (uint32_t k = 0; k < 4u; k++)
                if (b * 4u + k < L) out[b * 4u + k] = (uint8_t)((v >> (6u - 2u * k)) & 3u);
        } else {
            const uint32_t c[3] = {v / 25u, (v / 5u) % 5u, v % 5u};
            bool no = v >= 125u;
            for (uint32_t k = 0; k < 3u; k++) {
                if (b * 3u + k < L) out[b * 3u + k] = (uint8_t)min(c[k], 4u);
                else no |= c[k] != 0;
            }
            if (no) bad[OV_BAD_ROW] = 1;
        }
    }
}

// the given order is a permutation of 1 .. R: every number in range and met once
static __global__ void __launch_bounds__(OV_TPB) k_ov_perm(const uint32_t *__restrict__ order, uint64_t R, uint32_t *__restrict__ seen, uint32_t *__restrict__ bad) {
    const uint64_t j = (uint64_t)blockIdx.x * OV_TPB + threadIdx.x;
    if (j >= R) return;
    const uint32_t v = order[j];
    if (v < 1 || v > R) bad[OV_BAD_RANGE] = 1;
    else if (atomicExch(seen + v, 1u)) bad[OV_BAD_TWICE] = 1;
}

// eq[j] = the read at place j equals the one at j + 1; a read followed by a smaller one is reported
static __global__ void __launch_bounds__(OV_TPB) k_ov_adjacent(const uint8_t *__restrict__ sym, uint32_t stride, uint32_t L, const uint32_t *__restrict__ order, uint64_t R,
                                                               uint8_t *__restrict__ eq, uint32_t *__restrict__ bad) {
    const uint64_t j = (uint64_t)blockIdx.x * OV_TPB + threadIdx.x;
    if (j >= R) return;
    uint8_t same = 0;
    if (j + 1 < R) {
        const uint32_t a = order[j], b = order[j + 1];
        if (a >= 1 && a <= R && b >= 1 && b <= R) {     // (the permutation check reports the rest)
            const int c = ov_cmp(sym + (uint64_t)(a - 1) * stride, 0, sym + (uint64_t)(b - 1) * stride, 0, L);
            if (c > 0) bad[OV_BAD_SORT] = 1;
            same = c == 0;
        }
    }
    eq[j] = same;
}

// a run of equal reads becomes a chain; its first read goes to P, its last to S (flags for the compaction)
static __global__ void __launch_bounds__(OV_TPB) k_ov_chains(const uint32_t *__restrict__ order, const uint8_t *__restrict__ eq, uint64_t R, uint32_t L,
                                                             uint32_t *__restrict__ nx, uint16_t *__restrict__ ov, uint8_t *__restrict__ keep_s, uint8_t *__restrict__ keep_p) {
    const uint64_t j = (uint64_t)blockIdx.x * OV_TPB + threadIdx.x;
    if (j >= R) return;
    const bool same = eq[j];
    if (same) {
        nx[order[j]] = order[j + 1];
        ov[order[j]] = (uint16_t)L;
    }
    keep_s[j] = !same;
    keep_p[j] = j == 0 || !eq[j - 1];
}

// the order's sort: rec = (the 24-bit key of symbols [8c, 8c + 8) of the read) << 32 | read; FIRST: the reads 1 .. R in turn
template <bool FIRST>
static __global__ void __launch_bounds__(OV_TPB) k_ov_keys(const uint8_t *__restrict__ sym, uint32_t stride, uint32_t chunk, uint64_t R, const uint64_t *__restrict__ in,
                                                           uint64_t *__restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * OV_TPB + threadIdx.x;
    if (j >= R) return;
    const uint32_t r = FIRST ? (uint32_t)(j + 1) : (uint32_t)in[j];
    const uint64_t w = ov_ld8(sym + (uint64_t)(r - 1) * stride, chunk * OV_CHUNK);     // (zero after symbol L - 1)
    uint64_t key = 0;
#pragma unroll
    for (uint32_t t = 0; t < 8u; t++) key = (key << 3) | ((w >> (56u - 8u * t)) & 7u);
    out[j] = (key << 32) | r;
}

static __global__ void __launch_bounds__(OV_TPB) k_ov_order_of(const uint64_t *__restrict__ rec, uint64_t R, uint32_t *__restrict__ order) {
    const uint64_t j = (uint64_t)blockIdx.x * OV_TPB + threadIdx.x;
    if (j < R) order[j] = (uint32_t)rec[j];
}

// ------------------------------------------------------------------------------------------------ kernels: the lists
struct OvFlag {         // a flag byte as 0 / 1, or its negation
    const uint8_t *p;
    uint32_t inv;
    __device__ uint32_t operator()(uint64_t i) const { return (p[i] ? 1u : 0u) ^ inv; }
};

// dst[off[j]] = src[j] where the flag (negated: inv) is set; off = the exclusive scan of those flags
static __global__ void __launch_bounds__(OV_TPB) k_ov_compact(const uint32_t *__restrict__ src, const uint8_t *__restrict__ flag, uint32_t inv,
                                                              const uint32_t *__restrict__ off, uint64_t n, uint64_t cap, uint32_t *__restrict__ dst) {
    const uint64_t j = (uint64_t)blockIdx.x * OV_TPB + threadIdx.x;
    if (j >= n) return;
    if (((flag[j] ? 1u : 0u) ^ inv) && off[j] < cap) dst[off[j]] = src[j];
}

// gs[c] = the first place of S whose symbol at `at` is c or more (gs[5] = n): S is sorted by the suffix from `at` on
static __global__ void __launch_bounds__(OV_TPB) k_ov_groups(const uint8_t *__restrict__ sym, uint32_t stride, uint32_t at, const uint32_t *__restrict__ S, uint64_t n,
                                                             uint32_t *__restrict__ gs) {
    const uint64_t j = (uint64_t)blockIdx.x * OV_TPB + threadIdx.x;
    if (j > n) return;
    const int prev = j == 0 ? -1 : (int)sym[(uint64_t)(S[j - 1] - 1) * stride + at];
    const int cur = j == n ? 5 : (int)sym[(uint64_t)(S[j] - 1) * stride + at];
    for (int c = prev + 1; c <= cur; c++) gs[c] = (uint32_t)j;
}

// ------------------------------------------------------------------------------------------------ kernels: a sweep
// first place in [lo, hi) of S whose suffix from i on is not below (UPPER: is above) that of row x
template <bool UPPER>
__device__ __forceinline__ uint32_t ov_bound_s(const uint8_t *__restrict__ sym, uint32_t stride, uint32_t i, uint32_t L, const uint32_t *__restrict__ S, uint32_t lo,
                                               uint32_t hi, const uint8_t *__restrict__ x) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const int c = ov_cmp(sym + (uint64_t)(S[mid] - 1) * stride, i, x, i, L - i);
        if (UPPER ? c <= 0 : c < 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ranks: per suffix the start of its run in the merged order, the five shares of the run, its rank inside its group's share;
// the first suffix of a run (rank 0 in the first group that takes part) writes the run's transition at the run's start
// RESET (the parallel rule): a run that is the first of its block -- no suffix below it in any group shares its first three
// symbols -- writes "the symbol order, then the run" with the reset bit (scanops.h ScoWeakOrder5Reset)
template <bool RESET>
static __global__ void __launch_bounds__(OV_TPB) k_ov_ranks(const uint8_t *__restrict__ sym, uint32_t stride, uint32_t i, uint32_t L, const uint32_t *__restrict__ S,
                                                            uint32_t n, const uint32_t *__restrict__ gs, uint32_t *__restrict__ base, uint32_t *__restrict__ lens,
                                                            uint32_t *__restrict__ rk, uint32_t *__restrict__ trans) {
    const uint32_t j = blockIdx.x * OV_TPB + threadIdx.x;
    if (j >= n) return;
    const uint8_t *x = sym + (uint64_t)(S[j] - 1) * stride;
    const uint32_t g = x[i - 1];
    uint32_t len[5], below[5], start = 0, mine = 0, first = 5;
#pragma unroll
    for (uint32_t h = 0; h < 5u; h++) {
        const uint32_t lo = gs[h], hi = gs[h + 1];
        const uint32_t lb = ov_bound_s<false>(sym, stride, i, L, S, lo, hi, x);
        below[h] = lb > lo ? lb : 0u;       // (place + 1 of the group's last suffix below the run; 0: none)
        uint32_t ub = lb;
        // most runs have no share in another group: one compare tells
        if (lb < hi && ov_cmp(sym + (uint64_t)(S[lb] - 1) * stride, i, x, i, L - i) == 0) ub = ov_bound_s<true>(sym, stride, i, L, S, lb + 1, hi, x);
        len[h] = ub - lb;
        start += lb - lo;
        if (h == g) mine = (j - lo) - (lb - lo);
        if (len[h] && first == 5u) first = h;
    }
    base[j] = start;
    rk[j] = mine;
#pragma unroll
    for (uint32_t h = 0; h < 5u; h++) lens[(uint64_t)h * n + j] = len[h];
    if (mine == 0 && first == g && start < n) {
        uint32_t w = sco_dense5(len);
        if (RESET) {
            bool head = true;
#pragma unroll
            for (uint32_t h = 0; h < 5u; h++)
                if (below[h] && ov_cmp(sym + (uint64_t)(S[below[h] - 1] - 1) * stride, i, x, i, OV_BLOCK_PREFIX) == 0) head = false;
            if (head) w = ScoWeakOrder5{}((uint32_t)SCO_WEAK5_SYMBOL_ORDER, w) | SCO_WEAK5_RESET;
        }
        trans[start] = w;
    }
}

// place: round r of a run emits the r-th suffix of every group with more than r of them, in the order of the groups in front of
// the run -- before this suffix come min(len_h, r) of every group and one more of every group with len_h > r that stands earlier
// The parallel rule.  OV_PLACE_RESET: `state` is the scan of the transitions `trans` with resets; a run that starts a block stands
// behind the symbol order.  OV_PLACE_CONCAT (the last two sweeps): a block is its groups' shares one after the other
enum { OV_PLACE_SERIAL, OV_PLACE_RESET, OV_PLACE_CONCAT };
template <int MODE>
static __global__ void __launch_bounds__(OV_TPB) k_ov_place(const uint32_t *__restrict__ S, uint32_t n, const uint8_t *__restrict__ sym, uint32_t stride, uint32_t i,
                                                            const uint32_t *__restrict__ base, const uint32_t *__restrict__ lens, const uint32_t *__restrict__ rk,
                                                            const uint32_t *__restrict__ state, const uint32_t *__restrict__ trans, uint32_t *__restrict__ merged,
                                                            uint32_t *__restrict__ mk, uint32_t *__restrict__ bad) {
    const uint32_t j = blockIdx.x * OV_TPB + threadIdx.x;
    if (j >= n) return;
    const uint32_t x = S[j], g = sym[(uint64_t)(x - 1) * stride + i - 1], b = base[j], r = rk[j];
    if (b >= n) {
        bad[OV_BAD_PLACE] = 1;
        return;
    }
    uint32_t w = SCO_WEAK5_SYMBOL_ORDER;
    if (MODE == OV_PLACE_SERIAL) w = state[b];
    if (MODE == OV_PLACE_RESET && !(trans[b] & SCO_WEAK5_RESET)) w = state[b] & ~SCO_WEAK5_RESET;
    const uint32_t wg = (w >> (3u * g)) & 7u;
    uint32_t k = MODE == OV_PLACE_CONCAT ? r : 0u;
#pragma unroll
    for (uint32_t h = 0; h < 5u; h++) {
        const uint32_t len = lens[(uint64_t)h * n + j];
        if (MODE == OV_PLACE_CONCAT) k += h < g ? len : 0u;
        else k += min(len, r) + ((len > r && ((w >> (3u * h)) & 7u) < wg) ? 1u : 0u);
    }
    if ((uint64_t)b + k >= n) {
        bad[OV_BAD_PLACE] = 1;
        return;
    }
    merged[b + k] = x;
    mk[b + k] = k;
}

// pairing.  A = the run in merged order, B = the class of the run in P (the prefixes of L - i symbols that equal the run's
// suffix; contiguous from lbP on), k = this suffix's place in A.  e(t) = B[t] exists and is the read of A[t]; t is an event if
// e(t) and t - 1 is none, so inside a streak of e the events alternate.  A[k] takes B[k - 1] after an event, B[k + 1] at an
// event, B[k] otherwise -- if that prefix exists.  An unpaired suffix leaves S for good if the cursor of :193 is at the end
// when it is met: no prefix of its class is left for it and no prefix above its class exists.
// DROP = false (the parallel rule): an unpaired suffix always stays.
template <bool DROP>
static __global__ void __launch_bounds__(OV_TPB) k_ov_pair(const uint8_t *__restrict__ sym, uint32_t stride, uint32_t i, uint32_t L, const uint32_t *__restrict__ merged,
                                                           const uint32_t *__restrict__ mk, uint32_t n, const uint32_t *__restrict__ P, uint32_t np,
                                                           uint32_t *__restrict__ nx, uint16_t *__restrict__ ov, uint8_t *__restrict__ keep, uint8_t *__restrict__ taken) {
    const uint32_t p = blockIdx.x * OV_TPB + threadIdx.x;
    if (p >= n) return;
    const uint32_t x = merged[p], k = mk[p], m = L - i;
    const uint8_t *sx = sym + (uint64_t)(x - 1) * stride;
    uint32_t lo = 0, hi = np;
    while (lo < hi) {           // the first prefix that is not below the suffix
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ov_cmp(sx, i, sym + (uint64_t)(P[mid] - 1) * stride, 0, m) > 0) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t lbp = lo;
    auto in_class = [&](uint64_t q) { return q < np && ov_cmp(sx, i, sym + (uint64_t)(P[q] - 1) * stride, 0, m) == 0; };
    // the streak of e that ends at k - 1 (k <= p: the run starts at p - k)
    uint32_t streak = 0;
    for (uint32_t t = k; t > 0; t--) {
        const uint64_t q = (uint64_t)lbp + t - 1;
        if (q >= np || P[q] != merged[p - (k - (t - 1))] || !in_class(q)) break;
        streak++;
    }
    const bool after = streak & 1u;
    const uint64_t q = (uint64_t)lbp + k;
    const bool here = in_class(q);
    uint64_t take = ~0ull;
    if (after) take = q - 1;
    else if (here && P[q] == x) take = in_class(q + 1) ? q + 1 : ~0ull;
    else if (here) take = q;
    uint8_t stays = 0;
    if (take != ~0ull) {
        nx[x] = P[take];
        ov[x] = (uint16_t)m;
        taken[take] = 1;
    } else {
        const bool dropped = DROP && !here && ov_cmp(sx, i, sym + (uint64_t)(P[np - 1] - 1) * stride, 0, m) >= 0;
        stays = !dropped;
    }
    keep[p] = stays;
}

// ------------------------------------------------------------------------------------------------ kernels: the merge in front of sweep L - 3
// The parallel generator merges the suffixes of three symbols with a compare of length 0 that never stops
// (SymbolsPackingFacility::compareSequences :278-293): it runs on into the packed rows behind the two reads.  The key of read x
// is so the sequence of the reads x + 1, x + 2, ..., here of their dense ranks in the sorted order; a read past R is below any.
// Two different reads never compare equal: the larger one's rows end first.
struct OvFollow {
    const uint32_t *rnk;        // rnk[x], x = 1 .. R: the number of distinct reads below read x
    uint32_t R;
    __device__ int cmp(uint32_t x, uint32_t y, uint32_t *past) const {
        if (x == y) return 0;
        for (uint64_t k = 1;; k++) {
            const uint64_t a = x + k, b = y + k;
            if (a > R || b > R) {
                *past += 1;
                return a > b ? -1 : 1;
            }
            const uint32_t ra = rnk[a], rb = rnk[b];
            if (ra != rb) return ra < rb ? -1 : 1;
        }
    }
};

static __global__ void __launch_bounds__(OV_TPB) k_ov_rank_of(const uint32_t *__restrict__ order, const uint32_t *__restrict__ runs_before, uint64_t R,
                                                              uint32_t *__restrict__ rnk) {
    const uint64_t j = (uint64_t)blockIdx.x * OV_TPB + threadIdx.x;
    if (j < R) rnk[order[j]] = runs_before[j];
}

static __global__ void __launch_bounds__(OV_TPB) k_ov_place_of(const uint32_t *__restrict__ S, uint32_t n, uint32_t *__restrict__ at) {
    const uint32_t j = blockIdx.x * OV_TPB + threadIdx.x;
    if (j < n) at[S[j]] = j;
}

// the scan of the prefix maxima over the shares (one group's suffixes of one block; contiguous in S): an element is a read
// number, with OV_SHARE_FIRST on a share's first; 0 is the identity
#define OV_SHARE_FIRST (1ull << 32)
struct OvShareIn {
    const uint8_t *sym;
    const uint32_t *S;
    uint32_t stride, from;      // from = i - 1: the group's symbol and the block's three
    __device__ uint64_t operator()(uint64_t j) const {
        const uint32_t x = S[j];
        const bool first = j == 0 || ov_cmp(sym + (uint64_t)(x - 1) * stride, from, sym + (uint64_t)(S[j - 1] - 1) * stride, from, OV_BLOCK_PREFIX + 1u) != 0;
        return (first ? OV_SHARE_FIRST : 0ull) | x;
    }
};
struct OvShareMax {
    OvFollow f;
    __device__ uint64_t operator()(uint64_t a, uint64_t b) const {
        if (b & OV_SHARE_FIRST) return b;
        const uint32_t x = (uint32_t)a, y = (uint32_t)b;
        uint32_t past = 0;
        const uint32_t m = !x ? y : !y ? x : f.cmp(y, x, &past) > 0 ? y : x;
        return (a & OV_SHARE_FIRST) | m;
    }
};
struct OvLeadStore {
    uint32_t *p;
    __device__ void operator()(uint64_t i, uint64_t v) const { p[i] = (uint32_t)v; }
};

// A share is cut into segments at its prefix maxima (lead[j]: the maximum up to j, a read; at[read]: its place in S).  The block's
// segments come out by the key of their first suffix, so in front of suffix j stand: its segment up to j, the share up to the
// segment, and of every other group's share the suffixes whose maximum is below this one's (the maxima of a share ascend: a
// search).  Counted (cnt[0]: compares, cnt[1]: those that ran past row R): every suffix but a share's first against the
// maximum before it, and the searches of a segment's first suffix.
static __global__ void __launch_bounds__(OV_TPB) k_ov_place_follow(const uint32_t *__restrict__ S, uint32_t n, const uint8_t *__restrict__ sym, uint32_t stride, uint32_t i,
                                                                   uint32_t L, const uint32_t *__restrict__ gs, const uint32_t *__restrict__ base,
                                                                   const uint32_t *__restrict__ lens, const uint32_t *__restrict__ rk, const uint32_t *__restrict__ lead,
                                                                   const uint32_t *__restrict__ at, OvFollow f, uint32_t *__restrict__ merged, uint32_t *__restrict__ mk,
                                                                   unsigned long long *__restrict__ cnt, uint32_t *__restrict__ bad) {
    const uint32_t j = blockIdx.x * OV_TPB + threadIdx.x;
    if (j >= n) return;
    const uint32_t x = S[j], b = base[j], r = rk[j], m = lead[j];
    const uint8_t *sx = sym + (uint64_t)(x - 1) * stride;
    const uint32_t g = sx[i - 1], pm = m >= 1 && m <= f.R ? at[m] : n;
    if (b >= n || r > j || pm > j || pm < j - r) {        // (never: the maximum of a share's part up to j lies inside it)
        bad[OV_BAD_PLACE] = 1;
        return;
    }
    const bool heads = pm == j;
    uint32_t compares = 0, past = 0, k = r;         // own share: its segments keep their order, so all that stood in front of j
    if (r > 0) {
        (void)f.cmp(x, lead[j - 1], &past);
        compares++;
    }
#pragma unroll
    for (uint32_t h = 0; h < 5u; h++) {
        const uint32_t len = lens[(uint64_t)h * n + j];
        if (h == g || !len) continue;
        const uint32_t first = ov_bound_s<false>(sym, stride, i, L, S, gs[h], gs[h + 1], sx);
        uint32_t lo = first, hi = first + len;
        if (hi > n) {
            bad[OV_BAD_PLACE] = 1;
            return;
        }
        while (lo < hi) {           // the first place of the share whose maximum is not below this one's
            const uint32_t mid = lo + ((hi - lo) >> 1);
            uint32_t p = 0;
            const int c = f.cmp(lead[mid], m, &p);
            if (heads) {
                compares++;
                past += p;
            }
            if (c < 0) lo = mid + 1;
            else hi = mid;
        }
        k += lo - first;
    }
    if (compares) atomicAdd(cnt, (unsigned long long)compares);
    if (past) atomicAdd(cnt + 1, (unsigned long long)past);
    if ((uint64_t)b + k >= n) {
        bad[OV_BAD_PLACE] = 1;
        return;
    }
    merged[b + k] = x;
    mk[b + k] = k;
}

// ------------------------------------------------------------------------------------------------ kernels: afterwards
static __global__ void __launch_bounds__(OV_TPB) k_ov_narrow(const uint16_t *__restrict__ ov, uint64_t n, uint8_t *__restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * OV_TPB + threadIdx.x;
    if (j < n) out[j] = (uint8_t)ov[j];
}

static __global__ void __launch_bounds__(OV_TPB) k_ov_prev(const uint32_t *__restrict__ nx, const uint16_t *__restrict__ ov, uint64_t R, uint16_t *__restrict__ prev) {
    const uint64_t j = (uint64_t)blockIdx.x * OV_TPB + threadIdx.x;
    if (j == 0 || j > R) return;
    const uint32_t n = nx[j];
    if (n && n <= R) prev[n] = ov[j];
}

// getBothSidesOverlappedReads :82-90
static __global__ void __launch_bounds__(OV_TPB) k_ov_both(const uint32_t *__restrict__ nx, const uint16_t *__restrict__ ov, const uint16_t *__restrict__ prev, uint64_t R,
                                                           uint32_t L, uint8_t *__restrict__ flags) {
    const uint64_t j = (uint64_t)blockIdx.x * OV_TPB + threadIdx.x;
    if (j == 0 || j > R) return;
    const bool succ = nx[j] != 0;
    const uint32_t po = prev[j];
    flags[j - 1] = (po && succ) || (succ && ov[j] == L) || po == L;
}

// ------------------------------------------------------------------------------------------------ host side
static int ov_fail(pgrc_ovl_ctx *o, const std::string &msg) { return dec_fail(o, PGRC_E_PARAM, "overlap: " + msg); }

// off[0 .. n] = the exclusive scan of the flags (negated: inv), off[n] = their count
static int ov_scan_flags(pgrc_ovl_ctx *o, const uint8_t *flag, uint32_t inv, uint64_t n, uint32_t *off) {
    HIP_TRY(o, (sco_device_scan<false, true>(o->stream, OvFlag{flag, inv}, n, ScoPlus{}, 0u, 0u, ScoStore<uint32_t>{off}, (uint32_t *)o->fold.p)));
    return PGRC_OK;
}

// the sorted order made on the device: a stable LSD sort of the read numbers by 8 symbols a time, last chunk first
static int ov_make_order(pgrc_ovl_ctx *o, uint64_t R, uint32_t L, uint32_t stride) {
    int e;
    if ((e = pgrc_bufs_unpooled(o, {{&o->rec[0], R * 8}, {&o->rec[1], R * 8}}))) return e;
    uint64_t *cur = (uint64_t *)o->rec[0].p, *oth = (uint64_t *)o->rec[1].p;
    const uint8_t *sym = (const uint8_t *)o->sym.p;
    const uint32_t chunks = (L + OV_CHUNK - 1) / OV_CHUNK;
    for (uint32_t c = chunks; c-- > 0;) {
        if (c + 1 == chunks) hipLaunchKernelGGL(k_ov_keys<true>, dim3(dec_grid(R, OV_TPB)), dim3(OV_TPB), 0, o->stream, sym, stride, c, R, (const uint64_t *)nullptr, cur);
        else hipLaunchKernelGGL(k_ov_keys<false>, dim3(dec_grid(R, OV_TPB)), dim3(OV_TPB), 0, o->stream, sym, stride, c, R, (const uint64_t *)cur, cur);
        HIP_TRY(o, hipGetLastError());
        uint64_t *sorted = nullptr;
        if ((e = pgrc_radix_sort_u64(o, cur, oth, R, 32, 32 + 3 * OV_CHUNK, o->sort_scratch, &sorted))) return dec_fail(o, e, "overlap: " + o->err);
        if (sorted != cur) std::swap(cur, oth);
    }
    hipLaunchKernelGGL(k_ov_order_of, dim3(dec_grid(R, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint64_t *)cur, R, (uint32_t *)o->order.p);
    HIP_TRY(o, hipGetLastError());
    return PGRC_OK;
}

// rows_on_device: in->packed_rows is memory of this device (pgovl_run_rows), copied where the host's rows are uploaded
static int ov_run(pgrc_ovl_ctx *o, const pgrc_ovl_input *in, pgrc_ovl_result *out, bool rows_on_device) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t R = in->n_reads, N1 = R + 1;
    const uint32_t L = in->read_len, symbols = in->symbols, width = in->overlap_width;
    const uint32_t rb = symbols == 4 ? (L + 3) / 4 : (L + 2) / 3;
    const uint32_t stride = ((L + 7u) & ~7u) + 8u;
    const uint32_t iters = (uint8_t)((double)L * in->stop_coef);           // uint_read_len_min of :145
    const uint32_t sweeps = iters > 1 ? iters - 1 : 0;
    const uint64_t n_left = iters > 1 ? iters : 1;
    const bool par = o->rule == PGRC_OVL_RULE_PARALLEL;
    const uint32_t tail_from = L - OV_BLOCK_PREFIX;        // the parallel rule (L >= 4): the first sweep that pairs whole blocks
    const bool follow = par && tail_from <= sweeps;         // ... is run, and the merge in front of it
    int e;
    if ((e = o->ev.ensure(o))) return e;
    if ((e = pgrc_bufs_unpooled(o, {{&o->rows, R * rb + 16}, {&o->sym, R * stride + 16}, {&o->nx, N1 * 4}, {&o->ov, N1 * 2}, {&o->ovout, N1}, {&o->order, R * 4},
                                    {&o->seen, N1 * 4}, {&o->eq, R}, {&o->s[0], R * 4}, {&o->s[1], R * 4}, {&o->p[0], R * 4}, {&o->p[1], R * 4}, {&o->base, R * 4},
                                    {&o->lens, R * 20}, {&o->rk, R * 4}, {&o->trans, R * 4 + 64}, {&o->merged, R * 4}, {&o->mk, R * 4}, {&o->keep, R}, {&o->taken, R},
                                    {&o->offs, N1 * 4}, {&o->offp, N1 * 4}, {&o->gs, 64}, {&o->fold, dec_a16(sco_scratch_elems(N1) * 8)}, {&o->words, OV_BAD_WORDS * 4 + 16}})))
        return e;
    if (par && (e = pgrc_bufs_unpooled(o, {{&o->rnk, N1 * 4}, {&o->lead, R * 4}, {&o->cnt, 16}}))) return e;
    const uint8_t *rows = (const uint8_t *)o->rows.p;
    uint8_t *sym = (uint8_t *)o->sym.p, *eq = (uint8_t *)o->eq.p, *keep = (uint8_t *)o->keep.p, *taken = (uint8_t *)o->taken.p;
    uint32_t *nx = (uint32_t *)o->nx.p, *order = (uint32_t *)o->order.p, *base = (uint32_t *)o->base.p, *lens = (uint32_t *)o->lens.p, *rk = (uint32_t *)o->rk.p;
    uint32_t *trans = (uint32_t *)o->trans.p, *merged = (uint32_t *)o->merged.p, *mk = (uint32_t *)o->mk.p, *offs = (uint32_t *)o->offs.p, *offp = (uint32_t *)o->offp.p;
    uint32_t *gs = (uint32_t *)o->gs.p, *bad = (uint32_t *)o->words.p;
    uint16_t *ov = (uint16_t *)o->ov.p;

    if (rows_on_device) HIP_TRY(o, hipMemcpyAsync(o->rows.p, in->packed_rows, R * rb, hipMemcpyDeviceToDevice, o->stream));
    else if ((e = dec_upload_host(o, o->rows.p, in->packed_rows, R * rb))) return e;
    if (in->sorted_order && (e = dec_upload_host(o, order, in->sorted_order, R * 4))) return e;
    HIP_TRY(o, hipMemsetAsync(sym, 0, R * stride + 16, o->stream));
    HIP_TRY(o, hipMemsetAsync(nx, 0, N1 * 4, o->stream));
    HIP_TRY(o, hipMemsetAsync(ov, 0, N1 * 2, o->stream));
    HIP_TRY(o, hipMemsetAsync(o->seen.p, 0, N1 * 4, o->stream));
    HIP_TRY(o, hipMemsetAsync(bad, 0, OV_BAD_WORDS * 4, o->stream));
    if (par) HIP_TRY(o, hipMemsetAsync(o->cnt.p, 0, 16, o->stream));
    const float ms_upload = dec_ms_since(t0);

    // the rows unpacked and checked, the order made or checked
    HIP_TRY(o, o->ev.record(0, o->stream));
    {
        const uint64_t total = R * rb;
        hipLaunchKernelGGL(k_ov_unpack, dim3((uint32_t)std::min<uint64_t>(dec_grid(total, OV_TPB), 1u << 20)), dim3(OV_TPB), 0, o->stream, rows, total, rb, symbols, L, stride, sym, bad);
        HIP_TRY(o, hipGetLastError());
    }
    if (in->sorted_order) hipLaunchKernelGGL(k_ov_perm, dim3(dec_grid(R, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint32_t *)order, R, (uint32_t *)o->seen.p, bad);
    else if ((e = ov_make_order(o, R, L, stride))) return e;
    hipLaunchKernelGGL(k_ov_adjacent, dim3(dec_grid(R, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint8_t *)sym, stride, L, (const uint32_t *)order, R, eq, bad);
    HIP_TRY(o, hipGetLastError());
    HIP_TRY(o, o->ev.record(1, o->stream));
    uint32_t h_bad[OV_BAD_WORDS] = {};
    HIP_TRY(o, hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(o, hipStreamSynchronize(o->stream));
    // nothing below follows a read number before the order is known to be a permutation of 1 .. R
    if (h_bad[OV_BAD_ROW]) return ov_fail(o, "a row byte that is no packing of the alphabet");
    if (h_bad[OV_BAD_RANGE]) return ov_fail(o, "sorted_order holds a number outside 1 .. " + std::to_string(R));
    if (h_bad[OV_BAD_TWICE]) return ov_fail(o, "sorted_order holds a read twice");
    if (h_bad[OV_BAD_SORT]) {
        if (!in->sorted_order) return dec_fail(o, PGRC_E_DEVICE, "overlap: the order made on the device is not sorted");
        return ov_fail(o, "sorted_order is not sorted: a read is followed by a smaller one");
    }
    const float ms_order = o->ev.ms(0, 1);

    // the start: chains of equal reads, P and S, the groups by the first symbol
    uint32_t *S = (uint32_t *)o->s[0].p, *S2 = (uint32_t *)o->s[1].p, *P = (uint32_t *)o->p[0].p, *P2 = (uint32_t *)o->p[1].p;
    HIP_TRY(o, o->ev.record(0, o->stream));
    if (follow) {       // the reads' dense ranks: the runs of equal reads that end in front of a place of the order
        if ((e = ov_scan_flags(o, eq, 1, R, offs))) return e;
        hipLaunchKernelGGL(k_ov_rank_of, dim3(dec_grid(R, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint32_t *)order, (const uint32_t *)offs, R, (uint32_t *)o->rnk.p);
        HIP_TRY(o, hipGetLastError());
    }
    hipLaunchKernelGGL(k_ov_chains, dim3(dec_grid(R, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint32_t *)order, (const uint8_t *)eq, R, L, nx, ov, keep, taken);
    HIP_TRY(o, hipGetLastError());
    if ((e = ov_scan_flags(o, keep, 0, R, offs)) || (e = ov_scan_flags(o, taken, 0, R, offp))) return e;
    hipLaunchKernelGGL(k_ov_compact, dim3(dec_grid(R, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint32_t *)order, (const uint8_t *)keep, 0u, (const uint32_t *)offs, R, R, S);
    hipLaunchKernelGGL(k_ov_compact, dim3(dec_grid(R, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint32_t *)order, (const uint8_t *)taken, 0u, (const uint32_t *)offp, R, R, P);
    HIP_TRY(o, hipGetLastError());
    uint32_t h_n[2] = {};
    HIP_TRY(o, hipMemcpyAsync(&h_n[0], offs + R, 4, hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(o, hipMemcpyAsync(&h_n[1], offp + R, 4, hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(o, hipStreamSynchronize(o->stream));
    uint64_t ns = h_n[0], np = h_n[1];
    if (ns != np || ns < 1 || ns > R) return dec_fail(o, PGRC_E_DEVICE, "overlap: " + std::to_string(ns) + " chain ends and " + std::to_string(np) + " chain heads");
    hipLaunchKernelGGL(k_ov_groups, dim3(dec_grid(ns + 1, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint8_t *)sym, stride, 0u, (const uint32_t *)S, ns, gs);
    HIP_TRY(o, hipGetLastError());
    HIP_TRY(o, o->ev.record(1, o->stream));
    HIP_TRY(o, hipEventSynchronize(o->ev.ev[1]));
    const float ms_start = o->ev.ms(0, 1);

    // the block of the result; the reads-left numbers are written as they come
    const uint64_t ov_at = dec_a16(N1 * 4), left_at = ov_at + dec_a16(N1 * width), total = left_at + dec_a16(n_left * 8);
    uint8_t *blk = nullptr;
    if (hipHostMalloc((void **)&blk, total) != hipSuccess) {
        (void)hipGetLastError();
        return dec_fail(o, PGRC_E_ALLOC, "overlap: hipHostMalloc(" + std::to_string(total) + ") failed");
    }
    uint64_t *left = (uint64_t *)(blk + left_at);
    const uint64_t duplicates = R - ns;
    uint64_t reads_left = ns, links = 0;
    left[0] = reads_left;

    // the sweeps
    float ms_merge = 0, ms_pair = 0, ms_compact = 0;
    uint32_t passes = 0;
    o->sweep_ms.assign(sweeps, 0.f);
    e = PGRC_OK;
    for (uint32_t i = 1; i <= sweeps && !e; i++) {
        if (ns == 0 || np == 0) {       // nothing can link any more (with P empty the reference empties S, to no effect)
            left[i] = reads_left;
            continue;
        }
        const uint32_t n = (uint32_t)ns, npp = (uint32_t)np;
        hipError_t he = hipMemsetAsync(trans, 0, (uint64_t)n * 4, o->stream);
        if (he == hipSuccess) he = hipMemsetAsync(taken, 0, npp, o->stream);
        if (he == hipSuccess) he = o->ev.record(0, o->stream);
        if (!par) {
            hipLaunchKernelGGL(k_ov_ranks<false>, dim3(dec_grid(n, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint8_t *)sym, stride, i, L, (const uint32_t *)S, n, (const uint32_t *)gs,
                               base, lens, rk, trans);
            if (he == hipSuccess)
                he = sco_device_scan<false, false>(o->stream, ScoLoad<uint32_t, uint32_t, ScoIdentity>{trans, ScoIdentity{}}, (uint64_t)n, ScoWeakOrder5{}, 0u,
                                                   (uint32_t)SCO_WEAK5_SYMBOL_ORDER, ScoStore<uint32_t>{trans}, (uint32_t *)o->fold.p);
            hipLaunchKernelGGL(k_ov_place<OV_PLACE_SERIAL>, dim3(dec_grid(n, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint32_t *)S, n, (const uint8_t *)sym, stride, i,
                               (const uint32_t *)base, (const uint32_t *)lens, (const uint32_t *)rk, (const uint32_t *)trans, (const uint32_t *)trans, merged, mk, bad);
        } else if (i < tail_from) {
            // the order of the groups starts anew with every block: the transitions keep their reset bits, the scan goes to offs
            hipLaunchKernelGGL(k_ov_ranks<true>, dim3(dec_grid(n, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint8_t *)sym, stride, i, L, (const uint32_t *)S, n, (const uint32_t *)gs,
                               base, lens, rk, trans);
            if (he == hipSuccess)
                he = sco_device_scan<false, false>(o->stream, ScoLoad<uint32_t, uint32_t, ScoIdentity>{trans, ScoIdentity{}}, (uint64_t)n, ScoWeakOrder5Reset{}, 0u,
                                                   (uint32_t)SCO_WEAK5_SYMBOL_ORDER, ScoStore<uint32_t>{offs}, (uint32_t *)o->fold.p);
            hipLaunchKernelGGL(k_ov_place<OV_PLACE_RESET>, dim3(dec_grid(n, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint32_t *)S, n, (const uint8_t *)sym, stride, i,
                               (const uint32_t *)base, (const uint32_t *)lens, (const uint32_t *)rk, (const uint32_t *)offs, (const uint32_t *)trans, merged, mk, bad);
        } else if (i == tail_from) {
            // a run is a block; its order is the merge by the rows that follow the reads
            const OvFollow f{(const uint32_t *)o->rnk.p, (uint32_t)R};
            uint32_t *lead = (uint32_t *)o->lead.p, *at = (uint32_t *)o->seen.p;
            hipLaunchKernelGGL(k_ov_ranks<false>, dim3(dec_grid(n, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint8_t *)sym, stride, i, L, (const uint32_t *)S, n, (const uint32_t *)gs,
                               base, lens, rk, trans);
            hipLaunchKernelGGL(k_ov_place_of, dim3(dec_grid(n, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint32_t *)S, n, at);
            if (he == hipSuccess)
                he = sco_device_scan<true, false>(o->stream, OvShareIn{(const uint8_t *)sym, (const uint32_t *)S, stride, i - 1u}, (uint64_t)n, OvShareMax{f}, (uint64_t)0,
                                                  (uint64_t)0, OvLeadStore{lead}, (uint64_t *)o->fold.p);
            hipLaunchKernelGGL(k_ov_place_follow, dim3(dec_grid(n, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint32_t *)S, n, (const uint8_t *)sym, stride, i, L, (const uint32_t *)gs,
                               (const uint32_t *)base, (const uint32_t *)lens, (const uint32_t *)rk, (const uint32_t *)lead, (const uint32_t *)at, f, merged, mk,
                               (unsigned long long *)o->cnt.p, bad);
        } else {
            // what is left was regrouped by dropping its first symbol: a block is its groups' shares one after the other
            hipLaunchKernelGGL(k_ov_ranks<false>, dim3(dec_grid(n, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint8_t *)sym, stride, i, L, (const uint32_t *)S, n, (const uint32_t *)gs,
                               base, lens, rk, trans);
            hipLaunchKernelGGL(k_ov_place<OV_PLACE_CONCAT>, dim3(dec_grid(n, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint32_t *)S, n, (const uint8_t *)sym, stride, i,
                               (const uint32_t *)base, (const uint32_t *)lens, (const uint32_t *)rk, (const uint32_t *)trans, (const uint32_t *)trans, merged, mk, bad);
        }
        if (he == hipSuccess) he = hipGetLastError();
        if (he == hipSuccess) he = o->ev.record(1, o->stream);
        uint32_t placed_bad = 0;
        if (he == hipSuccess) he = hipMemcpyAsync(&placed_bad, bad + OV_BAD_PLACE, 4, hipMemcpyDeviceToHost, o->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(o->stream);
        if (he == hipSuccess && placed_bad) {       // (never: the merged order is a permutation of S; nothing is paired from a broken one)
            e = dec_fail(o, PGRC_E_DEVICE, "overlap: sweep " + std::to_string(i) + ": a place outside the merged order");
            break;
        }
        if (par)
            hipLaunchKernelGGL(k_ov_pair<false>, dim3(dec_grid(n, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint8_t *)sym, stride, i, L, (const uint32_t *)merged, (const uint32_t *)mk,
                               n, (const uint32_t *)P, npp, nx, ov, keep, taken);
        else
            hipLaunchKernelGGL(k_ov_pair<true>, dim3(dec_grid(n, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint8_t *)sym, stride, i, L, (const uint32_t *)merged, (const uint32_t *)mk,
                               n, (const uint32_t *)P, npp, nx, ov, keep, taken);
        if (he == hipSuccess) he = hipGetLastError();
        if (he == hipSuccess) he = o->ev.record(2, o->stream);
        if (he != hipSuccess) {
            e = dec_fail(o, pgrc_hip_code(he), std::string("overlap: sweep: ") + hipGetErrorString(he));
            break;
        }
        if ((e = ov_scan_flags(o, keep, 0, n, offs)) || (e = ov_scan_flags(o, taken, 1, npp, offp))) break;
        he = hipMemcpyAsync(&h_n[0], offs + n, 4, hipMemcpyDeviceToHost, o->stream);
        if (he == hipSuccess) he = hipMemcpyAsync(&h_n[1], offp + npp, 4, hipMemcpyDeviceToHost, o->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(o->stream);
        if (he != hipSuccess) {
            e = dec_fail(o, pgrc_hip_code(he), std::string("overlap: sweep: ") + hipGetErrorString(he));
            break;
        }
        if (h_n[0] > n || h_n[1] > npp) {
            e = dec_fail(o, PGRC_E_DEVICE, "overlap: sweep " + std::to_string(i) + ": more left than there was");
            break;
        }
        hipLaunchKernelGGL(k_ov_compact, dim3(dec_grid(n, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint32_t *)merged, (const uint8_t *)keep, 0u, (const uint32_t *)offs, (uint64_t)n,
                           (uint64_t)h_n[0], S2);
        hipLaunchKernelGGL(k_ov_compact, dim3(dec_grid(npp, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint32_t *)P, (const uint8_t *)taken, 1u, (const uint32_t *)offp, (uint64_t)npp,
                           (uint64_t)h_n[1], P2);
        std::swap(S, S2);
        std::swap(P, P2);
        hipLaunchKernelGGL(k_ov_groups, dim3(dec_grid((uint64_t)h_n[0] + 1, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint8_t *)sym, stride, i, (const uint32_t *)S, (uint64_t)h_n[0], gs);
        he = hipGetLastError();
        if (he == hipSuccess) he = o->ev.record(3, o->stream);
        if (he == hipSuccess) he = hipEventSynchronize(o->ev.ev[3]);
        if (he != hipSuccess) {
            e = dec_fail(o, pgrc_hip_code(he), std::string("overlap: sweep: ") + hipGetErrorString(he));
            break;
        }
        const uint64_t made = np - h_n[1];
        links += made;
        reads_left -= made;
        left[i] = reads_left;
        ns = h_n[0];
        np = h_n[1];
        const float a = o->ev.ms(0, 1), b = o->ev.ms(1, 2), c = o->ev.ms(2, 3);
        ms_merge += a;
        ms_pair += b;
        ms_compact += c;
        o->sweep_ms[i - 1] = a + b + c;
        passes++;
    }
    if (e) {
        (void)hipStreamSynchronize(o->stream);
        (void)hipHostFree(blk);
        return e;
    }

    // the result: one page-locked block
    const auto t1 = std::chrono::steady_clock::now();
    hipError_t he = hipSuccess;
    if (width == 1) {
        hipLaunchKernelGGL(k_ov_narrow, dim3(dec_grid(N1, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint16_t *)ov, N1, (uint8_t *)o->ovout.p);
        he = hipGetLastError();
    }
    unsigned long long h_cnt[2] = {};
    if (he == hipSuccess && par) he = hipMemcpyAsync(h_cnt, o->cnt.p, sizeof(h_cnt), hipMemcpyDeviceToHost, o->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(blk, nx, N1 * 4, hipMemcpyDeviceToHost, o->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(blk + ov_at, width == 1 ? o->ovout.p : (void *)ov, N1 * width, hipMemcpyDeviceToHost, o->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(o->stream);
    if (he != hipSuccess) {
        (void)hipHostFree(blk);
        return dec_fail(o, pgrc_hip_code(he), std::string("overlap: copy down: ") + hipGetErrorString(he));
    }
    out->struct_size = sizeof(pgrc_ovl_result);
    out->sweeps = sweeps;
    out->n_reads = R;
    out->n_left = n_left;
    out->duplicates = duplicates;
    out->links = links;
    out->next_read = (const uint32_t *)blk;
    out->overlap = blk + ov_at;
    out->reads_left_after = left;
    o->R = R;
    o->L = L;
    o->symbols = symbols;
    o->rb = rb;
    o->have_run = true;
    o->info = pgrc_ovl_rule_info{};
    o->info.struct_size = sizeof(pgrc_ovl_rule_info);
    o->info.rule = o->rule;
    if (par) {
        o->info.blocks = symbols * symbols * symbols;
        o->info.tail_sweeps = sweeps >= tail_from ? sweeps - tail_from + 1 : 0;
        o->info.follower_compares = h_cnt[0];
        o->info.past_end_compares = h_cnt[1];
    }
    pgrc_ovl_timing &t = o->tm;
    t = pgrc_ovl_timing{};
    t.struct_size = sizeof(pgrc_ovl_timing);
    t.passes = passes;
    t.ms_upload = ms_upload;
    t.ms_order_device = ms_order;
    t.ms_start_device = ms_start;
    t.ms_merge_device = ms_merge;
    t.ms_pair_device = ms_pair;
    t.ms_compact_device = ms_compact;
    t.ms_download = dec_ms_since(t1);
    t.ms_call = dec_ms_since(t0);
    t.bytes_up = (rows_on_device ? 0 : R * rb) + (in->sorted_order ? R * 4 : 0);
    t.bytes_down = N1 * 4 + N1 * width;
    return PGRC_OK;
}

extern "C" {

int pgrc_ovl_create(int32_t device, pgrc_ovl_ctx **out) {
    if (!out) return PGRC_E_PARAM;
    *out = nullptr;
    pgrc_ovl_ctx *o = new pgrc_ovl_ctx();
    const int e = pgrc_stage_open(o, device, &g_ov_create_err);
    if (e) delete o;
    else *out = o;
    return e;
}

void pgrc_ovl_destroy(pgrc_ovl_ctx *o) {
    if (!o) return;
    PgrcDeviceScope scope(o->device);
    (void)hipStreamSynchronize(o->stream);
    dec_free_all(ov_bufs(o));
    pgrc_buf_free(o->sort_scratch);
    o->ev.release();
    pgrc_stage_close(o);
    delete o;
}

const char *pgrc_ovl_last_error(const pgrc_ovl_ctx *o) { return o ? o->err.c_str() : g_ov_create_err.c_str(); }

}   // extern "C"

int pgovl_device(const pgrc_ovl_ctx *o) { return o->device; }
uint64_t pgovl_run_serial(const pgrc_ovl_ctx *o) { return o->have_run ? o->run_serial : 0; }

int pgovl_run_rows(pgrc_ovl_ctx *o, const pgrc_ovl_input *in, pgrc_ovl_result *out, bool rows_on_device) {
    if (!o) return PGRC_E_PARAM;
    if (!out) return ov_fail(o, "out is NULL");
    *out = pgrc_ovl_result{};
    o->have_run = false;        // the last run's graph goes whatever becomes of this one
    o->run_serial++;
    if (!in) return ov_fail(o, "in is NULL");
    if (in->struct_size != sizeof(pgrc_ovl_input)) return ov_fail(o, "struct_size is not sizeof(pgrc_ovl_input)");
    if (in->read_len < 1 || in->read_len > 255) return ov_fail(o, "the read length must be in [1, 255]");
    if (in->symbols != 4 && in->symbols != 5) return ov_fail(o, "the alphabet has 4 (ACGT) or 5 (ACGNT) symbols");
    if (in->overlap_width != 1 && in->overlap_width != 2) return ov_fail(o, "an overlap has 1 or 2 bytes");
    if (in->n_reads < 1 || in->n_reads > 0xFFFFFFFEull) return ov_fail(o, "the reads' count must be in [1, 2^32 - 2]");
    if (!(in->stop_coef >= 0.0 && in->stop_coef <= 1.0)) return ov_fail(o, "the stop coefficient must be in [0, 1]");
    if (!in->packed_rows) return ov_fail(o, "packed_rows is NULL");
    if (o->rule == PGRC_OVL_RULE_PARALLEL && in->read_len <= OV_BLOCK_PREFIX) return ov_fail(o, "the rule of the parallel generator needs a read length of at least 4");
    PGRC_ON_DEVICE(o);
    const int e = ov_run(o, in, out, rows_on_device);
    if (e) {
        (void)hipStreamSynchronize(o->stream);
        *out = pgrc_ovl_result{};
    }
    return e;
}

// getBothSidesOverlappedReads of the last run into o->flags, queued on the stream
static int ov_both_sides_queue(pgrc_ovl_ctx *o) {
    const uint64_t R = o->R, N1 = R + 1;
    int e;
    if ((e = pgrc_bufs_unpooled(o, {{&o->prev, N1 * 2}, {&o->flags, R}}))) return e;
    HIP_TRY(o, hipMemsetAsync(o->prev.p, 0, N1 * 2, o->stream));
    hipLaunchKernelGGL(k_ov_prev, dim3(dec_grid(N1, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint32_t *)o->nx.p, (const uint16_t *)o->ov.p, R, (uint16_t *)o->prev.p);
    hipLaunchKernelGGL(k_ov_both, dim3(dec_grid(N1, OV_TPB)), dim3(OV_TPB), 0, o->stream, (const uint32_t *)o->nx.p, (const uint16_t *)o->ov.p, (const uint16_t *)o->prev.p, R, o->L,
                       (uint8_t *)o->flags.p);
    HIP_TRY(o, hipGetLastError());
    return PGRC_OK;
}

// pgrc_ovl_assemble; list_stays: the reads list is left on the device (pgasm_run_device_resident; rlistctx.h)
int pgovl_assemble(pgrc_ovl_ctx *o, pgrc_asm_ctx *a, const uint32_t *index_mapping, pgrc_asm_result *res, bool list_stays) {
    if (!o) return PGRC_E_PARAM;
    if (!a || !res) return ov_fail(o, "asm_ctx or asm_result is NULL");
    *res = pgrc_asm_result{};
    if (!o->have_run) return dec_fail(o, PGRC_E_STATE, "overlap: no run has succeeded on this context");
    if (pgasm_device(a) != o->device) return ov_fail(o, "the two contexts are on different devices");
    {
        PGRC_ON_DEVICE(o);
        HIP_TRY(o, hipStreamSynchronize(o->stream));        // (a run leaves its stream idle; both_sides may have used it since)
    }
    pgrc_asm_input in{};
    in.struct_size = sizeof(in);
    in.read_len = o->L;
    in.symbols = o->symbols;
    in.overlap_width = 2;
    in.n_reads = o->R;
    in.packed_rows = (const uint8_t *)o->rows.p;
    in.next_read = (const uint32_t *)o->nx.p;
    in.overlap = o->ov.p;
    in.index_mapping = index_mapping;
    const int e = list_stays ? pgasm_run_device_resident(a, &in, res) : pgasm_run_device(a, &in, res);
    if (e) return dec_fail(o, e, std::string("overlap: ") + (pgrc_asm_last_error(a) ? pgrc_asm_last_error(a) : ""));
    return PGRC_OK;
}

int pgovl_both_sides_device(pgrc_ovl_ctx *o, const uint8_t **d_flags, uint64_t *R) {
    if (!o || !d_flags || !R) return PGRC_E_PARAM;
    if (!o->have_run) return dec_fail(o, PGRC_E_STATE, "overlap: no run has succeeded on this context");
    PGRC_ON_DEVICE(o);
    int e;
    if ((e = ov_both_sides_queue(o))) return e;
    HIP_TRY(o, hipStreamSynchronize(o->stream));
    *d_flags = (const uint8_t *)o->flags.p;
    *R = o->R;
    return PGRC_OK;
}

extern "C" {

int pgrc_ovl_run(pgrc_ovl_ctx *o, const pgrc_ovl_input *in, pgrc_ovl_result *out) { return pgovl_run_rows(o, in, out, false); }

void pgrc_ovl_free_result(pgrc_ovl_result *r) {
    if (!r) return;
    if (r->next_read) (void)hipHostFree(const_cast<uint32_t *>(r->next_read));
    *r = pgrc_ovl_result{};
}

int pgrc_ovl_both_sides(pgrc_ovl_ctx *o, uint8_t *flags) {
    if (!o) return PGRC_E_PARAM;
    if (!flags) return ov_fail(o, "flags is NULL");
    if (!o->have_run) return dec_fail(o, PGRC_E_STATE, "overlap: no run has succeeded on this context");
    PGRC_ON_DEVICE(o);
    const int e = ov_both_sides_queue(o);
    return e ? e : dec_download_host(o, flags, o->flags.p, o->R);
}

int pgrc_ovl_assemble(pgrc_ovl_ctx *o, pgrc_asm_ctx *a, const uint32_t *index_mapping, pgrc_asm_result *res) {
    return pgovl_assemble(o, a, index_mapping, res, false);
}

int pgrc_ovlrule_set(pgrc_ovl_ctx *o, uint32_t rule) {
    if (!o) return PGRC_E_PARAM;
    if (rule != PGRC_OVL_RULE_SERIAL && rule != PGRC_OVL_RULE_PARALLEL) return ov_fail(o, "the rule is PGRC_OVL_RULE_SERIAL or PGRC_OVL_RULE_PARALLEL");
    o->rule = rule;
    return PGRC_OK;
}

int pgrc_ovlrule_get_info(pgrc_ovl_ctx *o, pgrc_ovl_rule_info *out) {
    if (!o) return PGRC_E_PARAM;
    if (!out || out->struct_size != sizeof(pgrc_ovl_rule_info)) return dec_fail(o, PGRC_E_PARAM, "overlap: rule info is NULL or struct_size is not sizeof(pgrc_ovl_rule_info)");
    if (!o->have_run) return dec_fail(o, PGRC_E_STATE, "overlap: no run has succeeded on this context");
    *out = o->info;
    return PGRC_OK;
}

int pgrc_ovl_get_timing(pgrc_ovl_ctx *o, pgrc_ovl_timing *out) {
    if (!o) return PGRC_E_PARAM;
    if (!out || out->struct_size != sizeof(pgrc_ovl_timing)) return dec_fail(o, PGRC_E_PARAM, "timing is NULL or struct_size is not sizeof(pgrc_ovl_timing)");
    if (!o->have_run) return dec_fail(o, PGRC_E_STATE, "overlap: no run has succeeded on this context");
    *out = o->tm;
    return PGRC_OK;
}

int pgrc_ovl_get_sweep_ms(pgrc_ovl_ctx *o, float *ms, uint32_t n) {
    if (!o) return PGRC_E_PARAM;
    if (!ms && n) return ov_fail(o, "ms is NULL");
    if (!o->have_run) return dec_fail(o, PGRC_E_STATE, "overlap: no run has succeeded on this context");
    for (uint32_t k = 0; k < n && k < o->sweep_ms.size(); k++) ms[k] = o->sweep_ms[k];
    return PGRC_OK;
}

}   // extern "C"
