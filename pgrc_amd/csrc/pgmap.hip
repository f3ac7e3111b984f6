// pgmap.hip -- the matches of a pseudogenome-vs-pseudogenome call turned into the archive's mapped form on gfx950.
//
// Reference behaviour restated (not translated): SimplePgMatcher::markAndRemoveExactMatches, matching/SimplePgMatcher.cpp:69-148,
// with correctDestPositionDueToRevComplMatching (:58-61) and resolveMappingCollisionsInTheSameText (:157-171).  The reference
// sorts the matches, walks them once with a running position `pos` (a match that starts before pos is trimmed to pos, one that
// ends before it or gets shorter than minMatchLength is skipped), writes one '%' per kept match and compacts the text with
// memmove.  Here:
//   k_pm_norm      the two corrections per match, input checks                         -> (dst, src, len) per match
//   radix.hip      three stable pair sorts over the bits in use, len, then src, then dst: the order of TextMatch::operator<
//   k_pm_uniq      equal neighbours and matches below min_len drop out (the loop skips those without touching pos);
//                  k_pm_compact packs the rest: dst, src, e = dst + len, t = e - min_len
//   the greedy pass: with pos = p, match i is kept iff p <= t_i, and then pos = e_i.  So the kept matches are the path from
//                  match 0 through next(i) = the first j > i with t_j >= e_i.  A match i with some k < i, t_k >= e_i is never
//                  kept (k kept: pos >= e_k > t_i from then on; k skipped: pos > t_k >= e_i > t_i already), and for every other
//                  i the first j > i with t_j >= e_i is the first j AT ALL whose prefix maximum of t reaches e_i: one scan
//                  (scanops.h, operator max) and one binary search per match (k_pm_next), however many matches pile up inside
//                  a long one.  k_pm_jump marks the path by pointer jumping, ceil(log2(n)) passes, no host round trip.
//   k_pm_marks .. k_pm_streams   the kept matches in order, trimmed to their predecessor's end: d', s', L'; scans of L' and of the
//                  byte-frugal widths place every mark in the mapped text and every value in the lengths stream
//   k_pm_text      one lane, PM_LPT aligned 8-byte words of the MAPPED text: a binary search over the marks' mapped positions
//                  gives the literal run, the symbols come from the 2-bit text that the match call left in HBM (for an LQ / N
//                  text matched as its reverse complement: mirrored and complemented, 'N' from the N map) and leave as ASCII
// Integer work; the text kernel is a stream (0.25 bytes in, 1 byte out per symbol): no MFMA, no atomics, plain vector stores.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>

#include "scanops.h"

#include "ctx.h"
#include "devutil.h"
#include "memctx.h"
#include "pgrc_mem.h"
#include "varlenctx.h"

#define PM_TPB 256
#define PM_LPT 4               // 8-byte words of the mapped text per lane
#define PM_BAD_LEN 1u
#define PM_BAD_SRC 2u
#define PM_BAD_DST 4u

// ------------------------------------------------------------------------------------------------ device side

struct PmNorm {
    const pgrc_text_match *in;
    uint64_t n, N, N2;
    uint32_t dest_is_src, rev_compl;
    uint64_t *dst, *src, *len, *key, *idx;
    uint32_t *bad;
};

__global__ void __launch_bounds__(PM_TPB) k_pm_norm(const PmNorm a) {
    const uint64_t i = (uint64_t)blockIdx.x * PM_TPB + threadIdx.x;
    if (i >= a.n) return;
    const pgrc_text_match tm = a.in[i];
    uint64_t src = tm.pos_src, len = tm.length, dst = tm.pos_dest;
    uint32_t bad = 0;
    if (len == 0) bad |= PM_BAD_LEN;
    if (len > a.N || src > a.N - len) bad |= PM_BAD_SRC;
    if (len > a.N2 || dst > a.N2 - len) bad |= PM_BAD_DST;
    if (bad) {
        atomicOr(a.bad, bad);                                  // (the call is refused: the values only have to stay in range)
        src = dst = len = 0;
    }
    if (a.rev_compl) dst = a.N2 - (dst + len);                 // :58-61
    if (a.dest_is_src) {                                       // :157-171
        if (src > dst) { const uint64_t x = src; src = dst; dst = x; }
        if (a.rev_compl && src + len > dst) {
            const uint64_t margin = (src + len - dst + 1) / 2;
            len -= margin;
            dst += margin;
        }
    }
    a.dst[i] = dst;
    a.src[i] = src;
    a.len[i] = len;
    a.key[i] = len;                                            // the least significant field of the order goes first
    a.idx[i] = i;
}

__global__ void __launch_bounds__(PM_TPB) k_pm_gather(const uint64_t *__restrict__ field, const uint64_t *__restrict__ idx, uint64_t n, uint64_t *__restrict__ key) {
    const uint64_t k = (uint64_t)blockIdx.x * PM_TPB + threadIdx.x;
    if (k < n) key[k] = field[idx[k]];
}

// flag bit 0: the match enters the greedy pass; bit 1: it differs from its predecessor in the order
__global__ void __launch_bounds__(PM_TPB)
k_pm_uniq(const uint64_t *__restrict__ idx, const uint64_t *__restrict__ dst, const uint64_t *__restrict__ src, const uint64_t *__restrict__ len, uint64_t n,
          uint64_t min_len, uint8_t *__restrict__ flag) {
    const uint64_t k = (uint64_t)blockIdx.x * PM_TPB + threadIdx.x;
    if (k >= n) return;
    const uint64_t i = idx[k];
    bool uniq = true;
    if (k > 0) {
        const uint64_t j = idx[k - 1];
        uniq = dst[i] != dst[j] || src[i] != src[j] || len[i] != len[j];
    }
    flag[k] = (uint8_t)((uniq && len[i] >= min_len ? 1u : 0u) | (uniq ? 2u : 0u));
}
struct PmBit0 {
    __device__ uint32_t operator()(uint8_t f) const { return f & 1u; }
};
struct PmBit1 {
    __device__ uint32_t operator()(uint8_t f) const { return (f >> 1) & 1u; }
};
struct PmMax {
    __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; }
};

__global__ void __launch_bounds__(PM_TPB)
k_pm_compact(const uint64_t *__restrict__ idx, const uint8_t *__restrict__ flag, const uint32_t *__restrict__ slot, const uint64_t *__restrict__ dst,
             const uint64_t *__restrict__ src, const uint64_t *__restrict__ len, uint64_t n, uint64_t min_len, uint64_t *__restrict__ ud,
             uint64_t *__restrict__ us, uint64_t *__restrict__ ue, uint64_t *__restrict__ ut) {
    const uint64_t k = (uint64_t)blockIdx.x * PM_TPB + threadIdx.x;
    if (k >= n || !(flag[k] & 1u)) return;
    const uint64_t i = idx[k], s = slot[k] - 1u, e = dst[i] + len[i];
    ud[s] = dst[i];
    us[s] = src[i];
    ue[s] = e;
    ut[s] = e - min_len;
}

// next(i), see the head of the file; nu = "none".  Match 0 starts the path.
__global__ void __launch_bounds__(PM_TPB)
k_pm_next(const uint64_t *__restrict__ ue, const uint64_t *__restrict__ pmax, uint64_t nu, uint32_t *__restrict__ jump, uint32_t *__restrict__ kept) {
    const uint64_t i = (uint64_t)blockIdx.x * PM_TPB + threadIdx.x;
    if (i > nu) return;
    uint64_t nx = nu;
    if (i < nu && !(i > 0 && pmax[i - 1] >= ue[i])) {
        const uint64_t e = ue[i];
        uint64_t lo = i + 1, hi = nu;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (pmax[mid] < e) lo = mid + 1;
            else hi = mid;
        }
        nx = lo;
    }
    jump[i] = (uint32_t)nx;
    kept[i] = i == 0 && nu ? 1u : 0u;
}

// one pass: a match known to be on the path marks the one 2^r steps on; every pointer doubles its reach (jin -> jout, so that a
// pass reads the pointers of one round only; a mark seen early only marks another match of the path).  Slot nu is the end.
__global__ void __launch_bounds__(PM_TPB) k_pm_jump(const uint32_t *__restrict__ jin, uint32_t *__restrict__ jout, uint32_t *kept, uint64_t nu) {
    const uint64_t i = (uint64_t)blockIdx.x * PM_TPB + threadIdx.x;
    if (i > nu) return;
    const uint32_t j = jin[i];
    if (__hip_atomic_load(kept + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_store(kept + j, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    jout[i] = jin[j];
}

__global__ void __launch_bounds__(PM_TPB)
k_pm_marks(const uint32_t *__restrict__ kept, const uint32_t *__restrict__ kslot, const uint64_t *__restrict__ ud, const uint64_t *__restrict__ us,
           const uint64_t *__restrict__ ue, uint64_t nu, uint64_t *__restrict__ md, uint64_t *__restrict__ ms, uint64_t *__restrict__ me) {
    const uint64_t i = (uint64_t)blockIdx.x * PM_TPB + threadIdx.x;
    if (i >= nu || !kept[i]) return;
    const uint64_t k = kslot[i] - 1u;
    md[k] = ud[i];
    ms[k] = us[i];
    me[k] = ue[i];
}

__device__ __forceinline__ uint32_t pm_frugal_bytes(uint64_t v) { return v < 128 ? 1u : (uint32_t)(64 - __clzll((long long)v) + 6) / 7u; }

// mark k trimmed to the end of mark k - 1 (:113-123): d', L', the offsets stream's entry s', the width of its length value
__global__ void __launch_bounds__(PM_TPB)
k_pm_shape(const uint64_t *__restrict__ md, const uint64_t *__restrict__ ms, const uint64_t *__restrict__ me, uint64_t marks, uint32_t rev_compl, uint64_t min_len,
           uint32_t width, uint64_t *__restrict__ dp, uint64_t *__restrict__ lp, uint8_t *__restrict__ nb, void *__restrict__ off) {
    const uint64_t k = (uint64_t)blockIdx.x * PM_TPB + threadIdx.x;
    if (k >= marks) return;
    const uint64_t p = k ? me[k - 1] : 0, d = md[k] > p ? md[k] : p;
    const uint64_t s = ms[k] + (rev_compl ? 0 : d - md[k]), L = me[k] - d;
    dp[k] = d;
    lp[k] = L;
    nb[k] = (uint8_t)pm_frugal_bytes(L - min_len);
    if (width == 4) ((uint32_t *)off)[k] = (uint32_t)s;
    else ((uint64_t *)off)[k] = s;
}

// the mark's place in the mapped text and its value of the lengths stream (utils/helper.h:209-219)
__global__ void __launch_bounds__(PM_TPB)
k_pm_streams(const uint64_t *__restrict__ dp, const uint64_t *__restrict__ lp, const uint64_t *__restrict__ cum, const uint64_t *__restrict__ nbpos, uint64_t marks,
             uint64_t min_len, uint64_t *__restrict__ mp, uint8_t *__restrict__ lens) {
    const uint64_t k = (uint64_t)blockIdx.x * PM_TPB + threadIdx.x;
    if (k >= marks) return;
    mp[k] = dp[k] - cum[k] + k;
    uint64_t v = lp[k] - min_len, at = nbpos[k];
    while (v >= 128) {
        lens[at++] = (uint8_t)(128 + v % 128);
        v /= 128;
    }
    lens[at] = (uint8_t)v;
}

struct PmText {
    const uint32_t *text;        // 2 bits per symbol
    const uint16_t *nmap;        // nullptr: no 'N'
    uint64_t N2;
    uint32_t mirror;             // the text in HBM is the reverse complement of the text being mapped
    const uint64_t *mp, *cum;    // per mark: its position in the mapped text; [marks + 1] exclusive sums of the lengths
    uint64_t marks, mapped_len, nwords;
    uint64_t *out;
};

// symbol x of the destination, x < N2
__device__ __forceinline__ uint32_t pm_byte(const PmText &a, uint64_t x) {
    const uint64_t y = a.mirror ? a.N2 - 1 - x : x;
    uint32_t c = (a.text[y >> 4] >> (2u * ((uint32_t)y & 15u))) & 3u;
    if (a.mirror) c = 3u - c;
    if (a.nmap && ((a.nmap[y >> 4] >> ((uint32_t)y & 15u)) & 1u)) return (uint32_t)'N';
    return code2ascii(c);
}
// symbols x .. x + 7, x + 8 <= N2: two packed words in, eight bytes out
__device__ __forceinline__ uint64_t pm_word(const PmText &a, uint64_t x) {
    const uint64_t y0 = a.mirror ? a.N2 - 8 - x : x;
    const uint32_t *p = a.text + (y0 >> 4);
    const uint32_t sh = (uint32_t)y0 & 15u;
    const uint32_t bits = funnel_r(p[0], p[1], sh * 2u) & 0xFFFFu;
    uint32_t nbits = 0;
    if (a.nmap) {
        const uint16_t *q = a.nmap + (y0 >> 4);
        nbits = ((((uint32_t)q[0] | ((uint32_t)q[1] << 16)) >> sh)) & 0xFFu;
    }
    uint64_t v = 0;
#pragma unroll
    for (uint32_t b = 0; b < 8; b++) {
        const uint32_t j = a.mirror ? 7u - b : b;
        uint32_t c = (bits >> (2u * j)) & 3u;
        if (a.mirror) c = 3u - c;
        const uint32_t ch = ((nbits >> j) & 1u) ? (uint32_t)'N' : code2ascii(c);
        v |= (uint64_t)ch << (8u * b);
    }
    return v;
}

__global__ void __launch_bounds__(PM_TPB) k_pm_text(const PmText a) {
    const uint64_t w0 = ((uint64_t)blockIdx.x * PM_TPB + threadIdx.x) * PM_LPT;
    if (w0 >= a.nwords) return;
    uint64_t k = 0;                                            // marks before the lane's first byte
    {
        uint64_t hi = a.marks;
        const uint64_t o = 8 * w0;
        while (k < hi) {
            const uint64_t mid = (k + hi) >> 1;
            if (a.mp[mid] < o) k = mid + 1;
            else hi = mid;
        }
    }
    for (uint32_t u = 0; u < PM_LPT; u++) {
        const uint64_t w = w0 + u;
        if (w >= a.nwords) break;
        const uint64_t o = 8 * w;
        // the fast path: all 8 bytes in literal run k
        if (o + 8 <= a.mapped_len && (k == a.marks || a.mp[k] >= o + 8)) {
            const uint64_t x = o - k + a.cum[k];
            if (x + 8 <= a.N2) {
                a.out[w] = pm_word(a, x);
                continue;
            }
        }
        uint64_t v = 0;
        for (uint32_t b = 0; b < 8; b++) {
            const uint64_t pos = o + b;
            uint32_t ch = 0;
            if (pos < a.mapped_len) {
                if (k < a.marks && a.mp[k] == pos) {
                    ch = (uint32_t)'%';
                    k++;
                } else {
                    const uint64_t x = pos - k + a.cum[k];
                    if (x < a.N2) ch = pm_byte(a, x);
                }
            }
            v |= (uint64_t)ch << (8u * b);
        }
        a.out[w] = v;
    }
}

// ------------------------------------------------------------------------------------------------ host side
//
// Of the match that went before, the mapping reads m->dst (the destination's words, N map and what kind of call it was),
// m->evs.tmp (the radix sort's scratch) and m->base->txt (the packed source): memctx.h.  Everything else it touches is m->pm / m->res.

static uint32_t pm_bits(uint64_t v) {
    uint32_t b = 0;
    while (b < 64 && (v >> b)) b++;
    return b;
}
static uint32_t pm_grid(uint64_t items) { return (uint32_t)std::max<uint64_t>(1, (items + PM_TPB - 1) / PM_TPB); }

// every {buffer, bytes} in turn, 64 bytes at least; the first error ends it
static int pm_ensure(pgrc_mem_ctx *m, std::initializer_list<std::pair<DevBuf *, uint64_t>> want) {
    for (const auto &w : want)
        if (int e = pgrc_buf_ensure(m->base, *w.first, (size_t)std::max<uint64_t>(w.second, 64))) return e;
    return PGRC_OK;
}

// What the phases of one pm_mark_and_remove call hand to each other; it lives on that function's stack
struct PmCall {
    const pgrc_text_match *matches;  // as handed over, on the host
    uint64_t n;
    uint64_t N, N2, min_len;
    uint32_t width;                  // bytes of an entry of the offsets stream
    bool rc, dis;                    // the match call's rev_compl and dest_is_src
    int part;                        // 0 .. 2: the mapped text stays in HBM, in that slot; < 0: it goes down to mapped_out
    char *mapped_out;
    uint64_t nu = 0, nuniq = 0;      // matches that enter the greedy pass; distinct matches
    uint64_t marks = 0;
    uint64_t tot[2] = {0, 0};        // matched symbols; bytes of the length values
    uint64_t mapped_len = 0;
    bool resident() const { return part >= 0; }
};

// ---- 1. normalise, sort by (dst, src, len), unique
static int pm_sort_unique(pgrc_mem_ctx *m, PmCall &k) {
    pgrc_match_ctx *c = m->base;
    PmBufs &b = m->pm;
    hipStream_t st = c->stream;
    const uint64_t n = k.n;
    int e;
    if ((e = pm_ensure(m, {{&b.in, n * sizeof(pgrc_text_match)}, {&b.f[0], n * 8}, {&b.f[1], n * 8}, {&b.f[2], n * 8}, {&b.key[0], n * 8}, {&b.idx[0], n * 8},
                           {&b.key[1], n * 8}, {&b.idx[1], n * 8}, {&b.flag, n}, {&b.slot, 2 * n * 4}}))) return e;
    uint64_t *f_dst = (uint64_t *)b.f[0].p, *f_src = (uint64_t *)b.f[1].p, *f_len = (uint64_t *)b.f[2].p;
    uint32_t *d_bad = (uint32_t *)b.small.p, *fold32 = (uint32_t *)b.fold.p;
    HIP_TRY(c, hipMemsetAsync(d_bad, 0, 4, st));
    HIP_TRY(c, hipMemcpyAsync(b.in.p, k.matches, n * sizeof(pgrc_text_match), hipMemcpyHostToDevice, st));
    uint64_t *kcur = (uint64_t *)b.key[0].p, *kalt = (uint64_t *)b.key[1].p, *icur = (uint64_t *)b.idx[0].p, *ialt = (uint64_t *)b.idx[1].p;
    PmNorm a;
    a.in = (const pgrc_text_match *)b.in.p;
    a.n = n; a.N = k.N; a.N2 = k.N2;
    a.dest_is_src = k.dis ? 1u : 0u;
    a.rev_compl = k.rc ? 1u : 0u;
    a.dst = f_dst; a.src = f_src; a.len = f_len; a.key = kcur; a.idx = icur;
    a.bad = d_bad;
    hipLaunchKernelGGL(k_pm_norm, dim3(pm_grid(n)), dim3(PM_TPB), 0, st, a);
    uint32_t bad = 0;
    HIP_TRY(c, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (bad)
        return mem_fail(m, PGRC_E_PARAM, std::string("mark_and_remove: a match ") + ((bad & PM_BAD_LEN) ? "of length 0" : (bad & PM_BAD_SRC) ? "reaches past the source's end" : "reaches past the destination's end"));
    // stable passes over the bits in use, least significant field first
    const uint64_t *fields[3] = {f_len, f_src, f_dst};
    const uint32_t fbits[3] = {pm_bits(std::min(k.N, k.N2)), pm_bits(k.N), pm_bits(k.N2)};
    for (int f = 0; f < 3; f++) {
        if (f) hipLaunchKernelGGL(k_pm_gather, dim3(pm_grid(n)), dim3(PM_TPB), 0, st, fields[f], (const uint64_t *)icur, n, kcur);
        uint64_t *ks = nullptr, *vs = nullptr;
        if ((e = pgrc_radix_sort_pairs_u64(c, kcur, kalt, icur, ialt, n, 0, fbits[f], m->evs.tmp, &ks, &vs))) return e;
        if (vs != icur) { std::swap(icur, ialt); std::swap(kcur, kalt); }
    }
    uint32_t *d_slot = (uint32_t *)b.slot.p, *d_uslot = d_slot + n;
    hipLaunchKernelGGL(k_pm_uniq, dim3(pm_grid(n)), dim3(PM_TPB), 0, st, (const uint64_t *)icur, (const uint64_t *)f_dst, (const uint64_t *)f_src,
                       (const uint64_t *)f_len, n, k.min_len, (uint8_t *)b.flag.p);
    HIP_TRY(c, (sco_scan<true>(st, (const uint8_t *)b.flag.p, d_slot, n, PmBit0(), ScoPlus(), 0u, fold32)));
    HIP_TRY(c, (sco_scan<true>(st, (const uint8_t *)b.flag.p, d_uslot, n, PmBit1(), ScoPlus(), 0u, fold32)));
    uint32_t cnt[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(&cnt[0], d_slot + (n - 1), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&cnt[1], d_uslot + (n - 1), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    k.nu = cnt[0];
    k.nuniq = cnt[1];
    if (k.nu) {
        if ((e = pm_ensure(m, {{&b.u[0], k.nu * 8}, {&b.u[1], k.nu * 8}, {&b.u[2], k.nu * 8}, {&b.u[3], k.nu * 8}}))) return e;
        hipLaunchKernelGGL(k_pm_compact, dim3(pm_grid(n)), dim3(PM_TPB), 0, st, (const uint64_t *)icur, (const uint8_t *)b.flag.p, (const uint32_t *)d_slot,
                           (const uint64_t *)f_dst, (const uint64_t *)f_src, (const uint64_t *)f_len, n, k.min_len, (uint64_t *)b.u[0].p, (uint64_t *)b.u[1].p,
                           (uint64_t *)b.u[2].p, (uint64_t *)b.u[3].p);
    }
    return PGRC_OK;
}

// ---- 2. the greedy pass as a path
static int pm_greedy_path(pgrc_mem_ctx *m, PmCall &k) {
    pgrc_match_ctx *c = m->base;
    PmBufs &b = m->pm;
    hipStream_t st = c->stream;
    const uint64_t nu = k.nu;
    const uint64_t *ud = (const uint64_t *)b.u[0].p, *us = (const uint64_t *)b.u[1].p, *ue = (const uint64_t *)b.u[2].p, *ut = (const uint64_t *)b.u[3].p;
    if (int e = pm_ensure(m, {{&b.pmax, nu * 8}, {&b.jump[0], (nu + 1) * 4}, {&b.jump[1], (nu + 1) * 4}, {&b.kept, (nu + 1) * 4}, {&b.slot, nu * 4},
                              {&b.m[0], nu * 8}, {&b.m[1], nu * 8}, {&b.m[2], nu * 8}})) return e;
    uint64_t *pmax = (uint64_t *)b.pmax.p;
    uint32_t *kept = (uint32_t *)b.kept.p, *kslot = (uint32_t *)b.slot.p;
    HIP_TRY(c, (sco_device_scan<true, false>(st, ScoLoad<uint64_t, uint64_t, ScoIdentity>{ut, ScoIdentity{}}, nu, PmMax(), (uint64_t)0, (uint64_t)0,
                                             ScoStore<uint64_t>{pmax}, (uint64_t *)b.fold.p)));
    uint32_t *jin = (uint32_t *)b.jump[0].p, *jout = (uint32_t *)b.jump[1].p;
    hipLaunchKernelGGL(k_pm_next, dim3(pm_grid(nu + 1)), dim3(PM_TPB), 0, st, ue, (const uint64_t *)pmax, nu, jin, kept);
    for (uint64_t reach = 1; reach < nu; reach <<= 1) {
        hipLaunchKernelGGL(k_pm_jump, dim3(pm_grid(nu + 1)), dim3(PM_TPB), 0, st, (const uint32_t *)jin, jout, kept, nu);
        std::swap(jin, jout);
    }
    HIP_TRY(c, (sco_scan<true>(st, (const uint32_t *)kept, kslot, nu, ScoIdentity(), ScoPlus(), 0u, (uint32_t *)b.fold.p)));
    uint32_t nk = 0;
    HIP_TRY(c, hipMemcpyAsync(&nk, kslot + (nu - 1), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    k.marks = nk;
    hipLaunchKernelGGL(k_pm_marks, dim3(pm_grid(nu)), dim3(PM_TPB), 0, st, (const uint32_t *)kept, (const uint32_t *)kslot, ud, us, ue, nu, (uint64_t *)b.m[0].p,
                       (uint64_t *)b.m[1].p, (uint64_t *)b.m[2].p);
    return PGRC_OK;
}

// ---- 3. the marks and the two streams
static int pm_streams(pgrc_mem_ctx *m, PmCall &k) {
    pgrc_match_ctx *c = m->base;
    PmBufs &b = m->pm;
    hipStream_t st = c->stream;
    const uint64_t marks = k.marks;
    int e;
    if ((e = pm_ensure(m, {{&b.dp, marks * 8}, {&b.len, marks * 8}, {&b.nb, marks}, {&b.cum, (marks + 1) * 8}, {&b.nbpos, (marks + 1) * 8}, {&b.mp, marks * 8},
                           {&b.off, marks * k.width}}))) return e;
    uint64_t *cum = (uint64_t *)b.cum.p, *nbpos = (uint64_t *)b.nbpos.p, *fold64 = (uint64_t *)b.fold.p;
    if (marks)
        hipLaunchKernelGGL(k_pm_shape, dim3(pm_grid(marks)), dim3(PM_TPB), 0, st, (const uint64_t *)b.m[0].p, (const uint64_t *)b.m[1].p, (const uint64_t *)b.m[2].p,
                           marks, k.rc ? 1u : 0u, k.min_len, k.width, (uint64_t *)b.dp.p, (uint64_t *)b.len.p, (uint8_t *)b.nb.p, b.off.p);
    HIP_TRY(c, (sco_sum_u64<false>(st, (const uint64_t *)b.len.p, marks, cum, fold64)));
    HIP_TRY(c, (sco_sum_u64<false>(st, (const uint8_t *)b.nb.p, marks, nbpos, fold64)));
    HIP_TRY(c, hipMemcpyAsync(&k.tot[0], cum + marks, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&k.tot[1], nbpos + marks, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (k.tot[0] > k.N2 || k.tot[1] > 10 * marks) return mem_fail(m, PGRC_E_DEVICE, "mark_and_remove: inconsistent marks");
    if ((e = pm_ensure(m, {{&b.lens, k.tot[1]}}))) return e;
    if (marks)
        hipLaunchKernelGGL(k_pm_streams, dim3(pm_grid(marks)), dim3(PM_TPB), 0, st, (const uint64_t *)b.dp.p, (const uint64_t *)b.len.p, (const uint64_t *)cum,
                           (const uint64_t *)nbpos, marks, k.min_len, (uint64_t *)b.mp.p, (uint8_t *)b.lens.p);
    return PGRC_OK;
}

// ---- 4. the mapped text
static int pm_text(pgrc_mem_ctx *m, PmCall &k) {
    pgrc_match_ctx *c = m->base;
    k.mapped_len = k.N2 - k.tot[0] + k.marks;                  // (every mark replaces at least one symbol: <= N2)
    const uint64_t nwords = (k.mapped_len + 7) / 8;
    DevBuf &text_buf = k.resident() ? m->res.text[k.part] : m->pm.out;
    if (int e = pm_ensure(m, {{&text_buf, nwords * 8}})) return e;
    if (!nwords) return PGRC_OK;
    PmText t;
    t.text = k.dis ? (const uint32_t *)c->txt.pg2[0].p : (const uint32_t *)m->dst.words.p;
    t.nmap = (!k.dis && m->dst.has_n) ? (const uint16_t *)m->dst.nmap.p : nullptr;
    t.N2 = k.N2;
    t.mirror = (!k.dis && k.rc) ? 1u : 0u;
    t.mp = (const uint64_t *)m->pm.mp.p;
    t.cum = (const uint64_t *)m->pm.cum.p;
    t.marks = k.marks;
    t.mapped_len = k.mapped_len;
    t.nwords = nwords;
    t.out = (uint64_t *)text_buf.p;
    hipLaunchKernelGGL(k_pm_text, dim3(pm_grid((nwords + PM_LPT - 1) / PM_LPT)), dim3(PM_TPB), 0, c->stream, t);
    HIP_TRY(c, hipGetLastError());
    return PGRC_OK;
}

// ---- 5. the downloads
static int pm_download(pgrc_mem_ctx *m, const PmCall &k, pgrc_mem_mapping *out) {
    hipStream_t st = m->base->stream;
    const auto t0 = std::chrono::steady_clock::now();
    uint8_t hdr[10];
    uint32_t nh = 0;
    for (uint64_t v = k.min_len;; v /= 128) {
        if (v >= 128) hdr[nh++] = (uint8_t)(128 + v % 128);
        else { hdr[nh++] = (uint8_t)v; break; }
    }
    const uint64_t off_bytes = k.marks * k.width, len_bytes = nh + k.tot[1];
    uint8_t *block = (uint8_t *)malloc((size_t)(off_bytes + len_bytes + 1));
    if (!block) return mem_fail(m, PGRC_E_ALLOC, "out of host memory");
    memcpy(block + off_bytes, hdr, nh);
    hipError_t he = hipSuccess;
    if (off_bytes) he = hipMemcpyAsync(block, m->pm.off.p, off_bytes, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && k.tot[1]) he = hipMemcpyAsync(block + off_bytes + nh, m->pm.lens.p, k.tot[1], hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && k.mapped_len && !k.resident()) he = hipMemcpyAsync(k.mapped_out, m->pm.out.p, k.mapped_len, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) { free(block); return mem_fail(m, pgrc_hip_code(he), std::string("mapping download: ") + hipGetErrorString(he)); }
    m->pm.ms[4] = dec_ms_since(t0);
    out->mapped_len = k.mapped_len;
    out->marks = k.marks;
    out->unique_matches = k.nuniq;
    out->matched_symbols = k.tot[0];
    out->map_off = block;
    out->map_off_bytes = off_bytes;
    out->map_len = block + off_bytes;
    out->map_len_bytes = len_bytes;
    return PGRC_OK;
}

// pgrc_mem_mark_and_remove (part < 0: the mapped text goes down to mapped_out) and pgrc_mem_mark_and_remove_resident (part
// 0 .. 2: it stays in HBM, in the context's slot `part`)
static int pm_mark_and_remove(pgrc_mem_ctx *m, const pgrc_text_match *matches, uint64_t count, uint32_t min_match_len, char *mapped_out,
                              uint64_t mapped_cap, int part, pgrc_mem_mapping *out) {
    if (!m || !out) return PGRC_E_PARAM;
    memset(out, 0, sizeof *out);
    const bool resident = part >= 0;
    if (resident) m->res.set[part] = false;                    // (a failed call leaves no text in the slot)
    if (!m->dst.ready || !m->src.have) return mem_fail(m, PGRC_E_STATE, "mark_and_remove: no destination (call pgrc_mem_match_texts first)");
    const uint64_t N = m->src.N, N2 = m->dst.n2;
    const uint64_t min_len = min_match_len == UINT32_MAX ? m->src.L : min_match_len;
    if (min_len == 0) return mem_fail(m, PGRC_E_PARAM, "mark_and_remove: min_match_len is 0");
    if (!resident && (mapped_cap < N2 || (N2 && !mapped_out))) return mem_fail(m, PGRC_E_PARAM, "mark_and_remove: mapped_out is smaller than the destination");
    if (count && !matches) return PGRC_E_PARAM;
    if (count >= 0xFFFFF000ull) return mem_fail(m, PGRC_E_PARAM, "mark_and_remove: too many matches");
    pgrc_match_ctx *c = m->base;
    PgrcDeviceScope dev_scope__(c->device);
    if (!dev_scope__.ok) return mem_fail(m, PGRC_E_NO_DEVICE, "hipSetDevice failed");
    int e = m->pm.ev.ensure(c);
    if (e) return e;
    auto &ev = m->pm.ev;
    hipStream_t st = c->stream;
    PmCall k{matches, count, N, N2, min_len, N <= UINT32_MAX ? 4u : 8u, m->dst.rev_compl, m->dst.dest_is_src, part, mapped_out};
    if ((e = pm_ensure(m, {{&m->pm.fold, sco_scratch_elems(std::max<uint64_t>(count, 1)) * 8}, {&m->pm.small, 64}}))) return e;
    HIP_TRY(c, ev.record(0, st));
    if (k.n && (e = pm_sort_unique(m, k))) return e;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, ev.record(1, st));
    if (k.nu && (e = pm_greedy_path(m, k))) return e;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, ev.record(2, st));
    if ((e = pm_streams(m, k))) return e;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, ev.record(3, st));
    if ((e = pm_text(m, k))) return e;
    HIP_TRY(c, ev.record(4, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if ((e = pm_download(m, k, out))) return e;
    for (int p = 0; p < 4; p++) m->pm.ms[p] = ev.ms(p, p + 1);
    if (resident) {
        m->res.len[part] = k.mapped_len;
        m->res.set[part] = true;
    }
    return PGRC_OK;
}

extern "C" {

void pgrc_mem_free_mapping(pgrc_mem_mapping *mp) {
    if (!mp) return;
    free(mp->map_off);                                         // (one block: the lengths stream lies behind the offsets)
    memset(mp, 0, sizeof *mp);
}

int pgrc_mem_mapping_timing(pgrc_mem_ctx *m, float ms[5]) {
    if (!m || !ms) return PGRC_E_PARAM;
    memcpy(ms, m->pm.ms, sizeof m->pm.ms);
    return PGRC_OK;
}

int pgrc_mem_mark_and_remove(pgrc_mem_ctx *m, const pgrc_text_match *matches, uint64_t count, uint32_t min_match_len, char *mapped_out,
                             uint64_t mapped_cap, pgrc_mem_mapping *out) {
    return pm_mark_and_remove(m, matches, count, min_match_len, mapped_out, mapped_cap, -1, out);
}

int pgrc_mem_mark_and_remove_resident(pgrc_mem_ctx *m, const pgrc_text_match *matches, uint64_t count, uint32_t min_match_len, int32_t part,
                                      pgrc_mem_mapping *out) {
    if (m && out && (part < 0 || part > 2)) {
        memset(out, 0, sizeof *out);
        return mem_fail(m, PGRC_E_PARAM, "mark_and_remove_resident: part must be 0 (HQ), 1 (LQ) or 2 (N)");
    }
    return pm_mark_and_remove(m, matches, count, min_match_len, nullptr, 0, part, out);
}

int pgrc_mem_encode_mapped(pgrc_mem_ctx *m, pgrc_varlen *v, void *coded_out, uint64_t cap, uint64_t *coded_len, uint64_t lens[3]) {
    if (!m) return PGRC_E_PARAM;
    if (!v || !coded_len || !lens) return mem_fail(m, PGRC_E_PARAM, "encode_mapped: the coder, coded_len or lens is NULL");
    *coded_len = 0;
    lens[0] = lens[1] = lens[2] = 0;
    if (!m->res.set[0] || !m->res.set[1])
        return mem_fail(m, PGRC_E_STATE, "encode_mapped: no resident HQ or LQ text (call pgrc_mem_mark_and_remove_resident for parts 1, 2 and 0 first)");
    if (v->device != m->base->device) return mem_fail(m, PGRC_E_PARAM, "encode_mapped: the coder is on another device");
    pgrc_varlen_part parts[3];
    for (int p = 0; p < 3; p++) {
        parts[p].len = m->res.set[p] ? m->res.len[p] : 0;       // (an unset N slot: an empty part)
        parts[p].ptr = m->res.text[p].p;
        parts[p].on_device = 1;
    }
    const int e = pgrc_varlen_encode(v, parts, 3, coded_out, cap, 0, coded_len);
    if (e) return mem_fail(m, e, std::string("encode_mapped: ") + pgrc_varlen_last_error(v));
    for (int p = 0; p < 3; p++) lens[p] = parts[p].len;
    return PGRC_OK;
}

} // extern "C"
