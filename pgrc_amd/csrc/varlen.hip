// varlen.hip -- the variable-length DNA coder of the joined mapped pseudogenomes on gfx950 (include/pgrc_varlen.h).
//
// Reference behaviour restated (not translated): PgHelpers::VarLenDNACoder::encode / ::decode, coders/VarLenDNACoder.cpp:55-120,
// over a book handed in by the caller (initUsing, :10-35).  The reference walks the text once: at pos it looks the next four
// bytes up (27 bits of them), then three, then two, emits the first code found -- or the one-symbol code -- and steps over
// it.  Here:
//   the look-up  Create demands that the book's symbols differ in their low three bits, so the reference's 128 MB table
//                shrinks to four direct tables indexed by three bits a symbol (4096 + 512 + 64 + 8 bytes, made on the host in
//                the reference's overwrite order) and every block holds them in LDS
//   the parse    step(pos) depends on src[pos, pos + 4) and n alone, and the parse is the orbit of 0 under pos -> pos +
//                step(pos).  A run of symbols is therefore a map {0..3} -> {0..3}: the offset at which a parse enters it to the
//                offset at which it leaves it (scanops.h ScoMap4).  A thread owns VL_RUN symbols and walks them from all four
//                entries at once, backwards (the exit and the count of position i are those of i + step(i));
//   k_vl_maps    sco_block_exclusive composes the threads' maps; per block: its map, and its number of codes for each of the
//                four entries
//   the scans    sco_device_scan over the blocks' maps gives every block its entry, and over the counts for that entry
//                (ScoPlus, u64) its place in the output
//   k_vl_emit    the same maps again, now with the entry known: every thread walks its run once from its entry, the codes are
//                staged in LDS and leave as whole 16-byte lines
//   decode       k_vl_declen: a thread sums the lengths of 16 codes (a 256-byte table in LDS), blocks sum theirs; one scan;
//                k_vl_expand stages the symbols in LDS and writes whole lines
// Integer work on streams; no MFMA, no atomics, no library kernel, plain vector stores.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "scanops.h"

#include "ctx.h"
#include "pgrc_varlen.h"
#include "varlenctx.h"

#define VL_TPB 256
#define VL_RUN 32                       // symbols of a thread (encode)
#define VL_TILE (VL_TPB * VL_RUN)       // symbols of a block
#define VL_DRUN 16                      // codes of a thread (decode)
#define VL_DTILE (VL_TPB * VL_DRUN)     // codes of a block: at most 4 x as many symbols
#define VL_WORDS (VL_RUN / 4 + 1)       // a thread's symbols and the look-ahead of its last window, as 32-bit words

// ------------------------------------------------------------------------------------------------ device side

__device__ __forceinline__ uint64_t vl_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

struct VlSrc {
    const uint8_t *p[3];
    uint64_t end[3];                    // where part k ends in the joined text (an absent part ends where it starts)
    uint64_t n;
};

__device__ __forceinline__ uint32_t vl_byte(const VlSrc &s, uint64_t pos) {
    if (pos >= s.n) return 0;
    if (pos < s.end[0]) return s.p[0][pos];
    if (pos < s.end[1]) return s.p[1][pos - s.end[0]];
    return s.p[2][pos - s.end[1]];
}

template <int S>
__device__ __forceinline__ void vl_take(const uint32_t (&d)[13], uint32_t sb, uint32_t (&w)[VL_WORDS]) {
#pragma unroll
    for (int j = 0; j < VL_WORDS; j++) w[j] = (uint32_t)((((uint64_t)d[S + j + 1] << 32) | d[S + j]) >> (8u * sb));
}

// the 36 bytes from P on, zero past the text's end.  A window inside one part comes as aligned 16-byte loads (every one of
// them holds a byte of the window, so none leaves the part's pages) shifted into place; the shift is the same for all threads
// of a part, whose runs lie 32 bytes apart.  A window across two parts or the text's end comes byte by byte.
__device__ __forceinline__ void vl_load(const VlSrc &s, uint64_t P, uint32_t (&w)[VL_WORDS]) {
    const int k = P < s.end[0] ? 0 : P < s.end[1] ? 1 : 2;
    const uint64_t start = k ? s.end[k - 1] : 0;
    if (P + 4 * VL_WORDS <= s.end[k]) {
        const uintptr_t addr = (uintptr_t)(s.p[k] + (P - start));
        const uint4 *a = reinterpret_cast<const uint4 *>(addr & ~(uintptr_t)15);
        const uint32_t sh = (uint32_t)(addr & 15);
        const uint4 q0 = a[0], q1 = a[1], q2 = a[2];
        uint32_t last = 0;
        if (sh > 12) last = reinterpret_cast<const uint32_t *>(a + 3)[0];
        const uint32_t d[13] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, last};
        switch (sh >> 2) {
        case 0: vl_take<0>(d, sh & 3, w); break;
        case 1: vl_take<1>(d, sh & 3, w); break;
        case 2: vl_take<2>(d, sh & 3, w); break;
        default: vl_take<3>(d, sh & 3, w); break;
        }
    } else {
#pragma unroll
        for (int j = 0; j < VL_WORDS; j++) {
            uint32_t x = 0;
            for (int b = 0; b < 4; b++) x |= vl_byte(s, P + 4 * j + b) << (8 * b);
            w[j] = x;
        }
    }
}

// what the window with index idx (its symbols' low three bits) gives `rem` symbols before the text's end: code | step << 8.
// rem <= 0: past the end, a step of 1 that emits nothing
__device__ __forceinline__ uint32_t vl_lookup(const VlTables &t, uint32_t idx, int rem) {
    if (rem >= 4) return t.e[idx];
    if (rem <= 0) return 1u << 8;
    if (rem >= 3) {
        const uint32_t c = t.t3[idx & 511];
        if (c) return c | 3u << 8;
    }
    if (rem >= 2) {
        const uint32_t c = t.t2[idx & 63];
        if (c) return c | 2u << 8;
    }
    return t.t1[idx & 7] | 1u << 8;
}

struct VlRunState {
    uint64_t lo, hi;                    // three bits a symbol: symbols 0 .. 19 and 16 .. 35 of the window
    uint64_t st;                        // step - 1 of position i in bits [2i, 2i + 2)
    uint32_t map;                       // entry e -> exit, ScoMap4's form
    uint32_t cnt;                       // codes of the run entered at e in bits [8e, 8e + 8)
    uint32_t bad;                       // one of the run's own bytes is no symbol of the book
};

__device__ __forceinline__ uint32_t vl_idx(const VlRunState &r, uint32_t i) {
    return (uint32_t)(i < 16 ? r.lo >> (3 * i) : r.hi >> (3 * (i - 16))) & 0xFFFu;
}

// left: symbols from the run's first position to the text's end (capped; 0 for a run past the end)
__device__ __forceinline__ void vl_run(const VlTables &t, const uint32_t (&w)[VL_WORDS], int left, VlRunState &r) {
    uint64_t symw;
    memcpy(&symw, t.sym, 8);
    uint32_t bad = 0;
    uint64_t g[VL_WORDS];
#pragma unroll
    for (int j = 0; j < VL_WORDS; j++) {
        const uint32_t x = w[j];
        g[j] = (x & 7u) | ((x >> 8) & 7u) << 3 | ((x >> 16) & 7u) << 6 | ((x >> 24) & 7u) << 9;
        if (j < VL_RUN / 4) {
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint32_t c = (x >> (8 * b)) & 0xFFu;
                const uint32_t want = (uint32_t)(symw >> (8u * (c & 7u))) & 0xFFu;
                if (4 * j + b < left && (c == 0 || c != want)) bad = 1;
            }
        }
    }
    r.lo = g[0] | g[1] << 12 | g[2] << 24 | g[3] << 36 | g[4] << 48;
    r.hi = g[4] | g[5] << 12 | g[6] << 24 | g[7] << 36 | g[8] << 48;
    r.bad = bad;
    uint64_t st = 0;
#pragma unroll
    for (int i = 0; i < VL_RUN; i++) {
        const uint32_t e = vl_lookup(t, vl_idx(r, i), left - i);
        st |= (uint64_t)((e >> 8) - 1u) << (2 * i);
    }
    r.st = st;
    // backwards: the exits and counts of positions i + 1 .. i + 4 in we / wc, lowest first
    uint32_t we = SCO_MAP4_IDENTITY, wc = 0;
#pragma unroll
    for (int i = VL_RUN - 1; i >= 0; i--) {
        const uint32_t s = (uint32_t)(st >> (2 * i)) & 3u;
        const uint32_t e0 = (we >> (2 * s)) & 3u;
        const uint32_t c0 = ((wc >> (8 * s)) & 0xFFu) + (i < left ? 1u : 0u);
        we = ((we << 2) | e0) & 0xFFu;
        wc = (wc << 8) | c0;
    }
    r.map = we;
    r.cnt = wc;
}

__device__ __forceinline__ void vl_tables_to_lds(VlTables &dst, const VlTables *src) {
    const uint4 *g = reinterpret_cast<const uint4 *>(src);
    uint4 *l = reinterpret_cast<uint4 *>(&dst);
    for (uint32_t i = threadIdx.x; i < sizeof(VlTables) / 16; i += VL_TPB) l[i] = g[i];
    __syncthreads();
}

// stage[shift, shift + count) -> out[gbase, gbase + count), where shift = the low four bits of out + gbase's address: whole
// aligned 16-byte lines, single bytes at both ends
__device__ __forceinline__ void vl_flush(const uint8_t *stage, uint32_t shift, uint8_t *out, uint64_t gbase, uint32_t count) {
    const uint32_t total = shift + count;
    uint8_t *line0 = out + gbase - shift;
    for (uint32_t c = threadIdx.x; 16 * c < total; c += VL_TPB) {
        if (16 * c >= shift && 16 * c + 16 <= total) {
            *reinterpret_cast<uint4 *>(line0 + 16 * c) = *reinterpret_cast<const uint4 *>(stage + 16 * c);
        } else {
            for (uint32_t j = 16 * c; j < 16 * c + 16; j++)
                if (j >= shift && j < total) line0[j] = stage[j];
        }
    }
}

__global__ void __launch_bounds__(VL_TPB) k_vl_maps(const VlSrc s, const VlTables *__restrict__ tab, uint32_t *__restrict__ bmap,
                                                    uint64_t *__restrict__ bcnt, uint32_t *bad) {
    __shared__ __align__(16) VlTables t;
    __shared__ uint32_t sm32[VL_TPB / 64];
    __shared__ uint64_t sm64[VL_TPB / 64];
    vl_tables_to_lds(t, tab);
    const uint64_t P = ((uint64_t)blockIdx.x * VL_TPB + threadIdx.x) * VL_RUN;
    const int left = P < s.n ? (int)vl_min(s.n - P, 64) : 0;
    uint32_t w[VL_WORDS];
    vl_load(s, P, w);
    VlRunState r;
    vl_run(t, w, left, r);
    uint32_t tot;
    const uint32_t pre = sco_block_exclusive<VL_TPB / 64>(r.map, ScoMap4{}, SCO_MAP4_IDENTITY, sm32, &tot);
    uint64_t pk = 0;                                        // the run's codes for each entry of the BLOCK, 16 bits each
#pragma unroll
    for (int eb = 0; eb < 4; eb++) pk |= (uint64_t)((r.cnt >> (8 * ((pre >> (2 * eb)) & 3u))) & 0xFFu) << (16 * eb);
    uint64_t ptot;
    sco_block_sum<VL_TPB / 64>(pk, sm64, &ptot);            // (at most VL_TILE = 8192 a field: no carry between them)
    if (threadIdx.x == 0) {
        bmap[blockIdx.x] = tot;
        bcnt[blockIdx.x] = ptot;
    }
    if (r.bad) *bad = 1;                                    // (every writer writes the same word: no atomic)
}

// block i's codes, given the map of everything before it
struct VlBlockCount {
    const uint64_t *bcnt;
    const uint32_t *bent;
    __device__ uint64_t operator()(uint64_t i) const { return (bcnt[i] >> (16 * (bent[i] & 3u))) & 0xFFFFu; }
};

__global__ void __launch_bounds__(VL_TPB) k_vl_emit(const VlSrc s, const VlTables *__restrict__ tab, const uint32_t *__restrict__ bent,
                                                    const uint64_t *__restrict__ bbase, uint8_t *__restrict__ out, uint64_t total) {
    __shared__ __align__(16) VlTables t;
    __shared__ __align__(16) uint8_t stage[VL_TILE + 16];
    __shared__ uint32_t sm32[VL_TPB / 64];
    vl_tables_to_lds(t, tab);
    const uint64_t P = ((uint64_t)blockIdx.x * VL_TPB + threadIdx.x) * VL_RUN;
    const int left = P < s.n ? (int)vl_min(s.n - P, 64) : 0;
    const uint32_t eb = bent[blockIdx.x] & 3u;              // the parse enters the block here (the map before it, applied to 0)
    const uint64_t gbase = bbase[blockIdx.x];
    uint32_t w[VL_WORDS];
    vl_load(s, P, w);
    VlRunState r;
    vl_run(t, w, left, r);
    uint32_t tot, btot;
    const uint32_t pre = sco_block_exclusive<VL_TPB / 64>(r.map, ScoMap4{}, SCO_MAP4_IDENTITY, sm32, &tot);
    const uint32_t entry = (pre >> (2 * eb)) & 3u;
    const uint32_t mine = (r.cnt >> (8 * entry)) & 0xFFu;
    const uint32_t off = sco_block_sum<VL_TPB / 64>(mine, sm32, &btot);
    const uint32_t shift = (uint32_t)((uintptr_t)(out + gbase) & 15);
    uint32_t o = shift + off;
    for (int pos = (int)entry; pos < VL_RUN && pos < left; pos += (int)((r.st >> (2 * pos)) & 3u) + 1) {
        if (o < sizeof stage) stage[o] = (uint8_t)vl_lookup(t, vl_idx(r, (uint32_t)pos), left - pos);
        o++;
    }
    __syncthreads();
    const uint64_t room = gbase < total ? total - gbase : 0;   // (the counts of both passes agree; the clamp keeps a text that
    vl_flush(stage, shift, out, gbase, (uint32_t)vl_min(btot, room));   // changed in between inside the output)
}

// ---- decode
__device__ __forceinline__ void vl_load_codes(const uint8_t *coded, uint64_t m, uint64_t c0, uint8_t (&c)[VL_DRUN], int &have) {
    have = c0 < m ? (int)vl_min(m - c0, VL_DRUN) : 0;
    if (have == VL_DRUN && ((uintptr_t)(coded + c0) & 15) == 0) {
        const uint4 q = *reinterpret_cast<const uint4 *>(coded + c0);
        memcpy(c, &q, 16);
    } else {
#pragma unroll
        for (int j = 0; j < VL_DRUN; j++) c[j] = j < have ? coded[c0 + j] : 0;
    }
}

__global__ void __launch_bounds__(VL_TPB) k_vl_declen(const uint8_t *__restrict__ coded, uint64_t m, const VlBook *__restrict__ book,
                                                      uint32_t *__restrict__ bsum) {
    __shared__ uint8_t len[256];
    __shared__ uint32_t sm32[VL_TPB / 64];
    len[threadIdx.x] = book->len[threadIdx.x];
    __syncthreads();
    uint8_t c[VL_DRUN];
    int have;
    vl_load_codes(coded, m, ((uint64_t)blockIdx.x * VL_TPB + threadIdx.x) * VL_DRUN, c, have);
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < VL_DRUN; j++) sum += j < have ? len[c[j]] : 0u;
    uint32_t tot;
    sco_block_sum<VL_TPB / 64>(sum, sm32, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(VL_TPB) k_vl_expand(const uint8_t *__restrict__ coded, uint64_t m, const VlBook *__restrict__ book,
                                                      const uint64_t *__restrict__ bbase, uint8_t *__restrict__ out, uint64_t total) {
    __shared__ __align__(16) VlBook bk;
    __shared__ __align__(16) uint8_t stage[4 * VL_DTILE + 16];
    __shared__ uint32_t sm32[VL_TPB / 64];
    {
        const uint4 *g = reinterpret_cast<const uint4 *>(book);
        uint4 *l = reinterpret_cast<uint4 *>(&bk);
        for (uint32_t i = threadIdx.x; i < sizeof(VlBook) / 16; i += VL_TPB) l[i] = g[i];
        __syncthreads();
    }
    uint8_t c[VL_DRUN];
    int have;
    vl_load_codes(coded, m, ((uint64_t)blockIdx.x * VL_TPB + threadIdx.x) * VL_DRUN, c, have);
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < VL_DRUN; j++) sum += j < have ? bk.len[c[j]] : 0u;
    uint32_t btot;
    const uint32_t off = sco_block_sum<VL_TPB / 64>(sum, sm32, &btot);
    const uint64_t gbase = bbase[blockIdx.x];
    const uint32_t shift = (uint32_t)((uintptr_t)(out + gbase) & 15);
    uint32_t o = shift + off;
#pragma unroll
    for (int j = 0; j < VL_DRUN; j++) {
        if (j < have) {
            const uint32_t x = bk.bytes[c[j]], l = bk.len[c[j]];
            for (uint32_t b = 0; b < l; b++)
                if (o + b < sizeof stage) stage[o + b] = (uint8_t)(x >> (8 * b));
            o += l;
        }
    }
    __syncthreads();
    const uint64_t room = gbase < total ? total - gbase : 0;
    vl_flush(stage, shift, out, gbase, (uint32_t)vl_min(btot, room));
}

// ------------------------------------------------------------------------------------------------ host side
static thread_local std::string g_vl_create_err;

static int vl_fail(pgrc_varlen *v, int code, const std::string &msg) {
    v->err = msg;
    return code;
}

static bool vl_is_device_ptr(const void *p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) == hipSuccess) return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
    (void)hipGetLastError();
    return false;
}

// The book and its tables.  The reference fills one table over 27-bit keys in index order, later codes over earlier ones,
// every empty code at key 0; `lut` is that table, sparse.
static int vl_parse_book(pgrc_varlen *v, const uint8_t *book, uint64_t book_bytes, std::string &err) {
    uint64_t nb = 0;
    while (nb < book_bytes && book[nb]) nb++;               // (readBook takes a C string)
    std::vector<std::string> codes(1);
    for (uint64_t i = 0; i < nb; i++) {
        if (book[i] == '\n') {
            codes.emplace_back();
            if (codes.size() > 256) { err = "more than 256 codes in the book"; return PGRC_E_PARAM; }
        } else {
            codes.back().push_back((char)book[i]);
            if (codes.back().size() > 4) { err = "code " + std::to_string(codes.size() - 1) + " is longer than 4 bytes"; return PGRC_E_PARAM; }
        }
    }
    if (codes[0].size() != 1) { err = "code 0 (the not-found value) must be one symbol"; return PGRC_E_PARAM; }
    bool is_sym[256] = {}, has_single[256] = {};
    for (const std::string &c : codes) {
        for (char ch : c) is_sym[(uint8_t)ch] = true;
        if (c.size() == 1) has_single[(uint8_t)c[0]] = true;
    }
    memset(&v->tab, 0, sizeof v->tab);
    memset(&v->book, 0, sizeof v->book);
    memset(v->t4, 0, sizeof v->t4);
    for (uint32_t s = 1; s < 256; s++) {
        if (!is_sym[s]) continue;
        if (!(s & 7)) {
            err = std::string("symbol '") + (char)s + "' of the book has the low three bits 0: in a window's fourth place it cannot be told from no byte";
            return PGRC_E_PARAM;
        }
        if (!has_single[s]) { err = std::string("symbol '") + (char)s + "' of the book has no one-symbol code"; return PGRC_E_PARAM; }
        if (v->tab.sym[s & 7]) {
            err = std::string("symbols '") + (char)v->tab.sym[s & 7] + "' and '" + (char)s + "' share their low three bits";
            return PGRC_E_PARAM;
        }
        v->tab.sym[s & 7] = (uint8_t)s;
    }
    v->ncodes = (uint32_t)codes.size();
    std::map<uint32_t, uint8_t> lut;
    for (uint32_t i = 0; i < v->ncodes; i++) {
        uint32_t key = 0;
        for (size_t b = 0; b < codes[i].size(); b++) key |= (uint32_t)(uint8_t)codes[i][b] << (8 * b);
        v->book.bytes[i] = key;
        v->book.len[i] = (uint8_t)codes[i].size();
        lut[key & 0x07FFFFFFu] = (uint8_t)i;
    }
    auto look = [&](uint32_t key) -> uint8_t {
        const auto it = lut.find(key);
        return it == lut.end() ? 0 : it->second;
    };
    const uint8_t *sym = v->tab.sym;
    for (uint32_t idx = 0; idx < 4096; idx++) {
        const uint32_t s0 = sym[idx & 7], s1 = sym[(idx >> 3) & 7], s2 = sym[(idx >> 6) & 7], s3 = sym[(idx >> 9) & 7];
        if (idx < 8 && s0) v->tab.t1[idx] = look(s0);
        if (idx < 64 && s0 && s1) v->tab.t2[idx] = look(s0 | s1 << 8);
        if (idx < 512 && s0 && s1 && s2) v->tab.t3[idx] = look(s0 | s1 << 8 | s2 << 16);
        if (s0 && s1 && s2 && s3) v->t4[idx] = look(s0 | s1 << 8 | s2 << 16 | (s3 & 7u) << 24);
    }
    for (uint32_t idx = 0; idx < 4096; idx++) {
        uint32_t e;
        if (v->t4[idx]) e = v->t4[idx] | 4u << 8;
        else if (v->tab.t3[idx & 511]) e = v->tab.t3[idx & 511] | 3u << 8;
        else if (v->tab.t2[idx & 63]) e = v->tab.t2[idx & 63] | 2u << 8;
        else e = v->tab.t1[idx & 7] | 1u << 8;
        v->tab.e[idx] = (uint16_t)e;
    }
    return PGRC_OK;
}

extern "C" {

uint64_t pgrc_varlen_bound(uint64_t n) { return n; }

void pgrc_varlen_destroy(pgrc_varlen *v) {
    if (!v) return;
    PgrcDeviceScope scope(v->device);
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    dec_free_all({&v->d_tab, &v->d_book, &v->d_src, &v->d_coded, &v->d_text, &v->d_bmap, &v->d_bent, &v->d_bcnt, &v->d_bsum, &v->d_bbase, &v->d_fold, &v->d_flag});
    v->ev.release();
    if (v->stream) (void)hipStreamDestroy(v->stream);
    delete v;
}

const char *pgrc_varlen_last_error(const pgrc_varlen *v) { return v ? v->err.c_str() : g_vl_create_err.c_str(); }

int pgrc_varlen_create(const void *book, uint64_t book_bytes, int32_t device, pgrc_varlen **out) {
    if (!out) return PGRC_E_PARAM;
    *out = nullptr;
    if (!book) { g_vl_create_err = "book is NULL"; return PGRC_E_PARAM; }
    pgrc_varlen *v = new pgrc_varlen();
    int e = vl_parse_book(v, (const uint8_t *)book, book_bytes, g_vl_create_err);
    if (e) { delete v; return e; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        g_vl_create_err = "no HIP device";
        delete v;
        return PGRC_E_NO_DEVICE;
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess) { g_vl_create_err = "hipGetDevice failed"; delete v; return PGRC_E_NO_DEVICE; }
    if (device >= ndev) { g_vl_create_err = "device " + std::to_string(device) + " does not exist"; delete v; return PGRC_E_NO_DEVICE; }
    v->device = device;
    PgrcDeviceScope scope(device);
    if (!scope.ok) e = PGRC_E_NO_DEVICE;
    if (!e && hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess) e = PGRC_E_DEVICE;
    if (!e && v->ev.ensure(v)) e = PGRC_E_DEVICE;
    if (!e) e = pgrc_buf_unpooled(v, v->d_tab, sizeof(VlTables));
    if (!e) e = pgrc_buf_unpooled(v, v->d_book, sizeof(VlBook));
    if (!e) e = pgrc_buf_unpooled(v, v->d_flag, 64);
    if (!e && (hipMemcpyAsync(v->d_tab.p, &v->tab, sizeof(VlTables), hipMemcpyHostToDevice, v->stream) != hipSuccess ||
               hipMemcpyAsync(v->d_book.p, &v->book, sizeof(VlBook), hipMemcpyHostToDevice, v->stream) != hipSuccess ||
               hipStreamSynchronize(v->stream) != hipSuccess))
        e = PGRC_E_DEVICE;
    if (e) {
        g_vl_create_err = v->err.empty() ? "HIP stream / event creation or the upload of the tables failed" : v->err;
        (void)hipGetLastError();
        pgrc_varlen_destroy(v);
        return e;
    }
    *out = v;
    return PGRC_OK;
}

int pgrc_varlen_timing(pgrc_varlen *v, pgrc_varlen_times *out) {
    if (!v || !out) return PGRC_E_PARAM;
    *out = v->tm;
    return PGRC_OK;
}

int pgrc_varlen_encode(pgrc_varlen *v, const pgrc_varlen_part *parts, uint32_t n_parts, void *out, uint64_t out_cap, int32_t out_on_device,
                       uint64_t *coded_len) {
    if (!v) return PGRC_E_PARAM;
    if (!coded_len) return vl_fail(v, PGRC_E_PARAM, "encode: coded_len is NULL");
    *coded_len = 0;
    if (n_parts > 3 || (n_parts && !parts)) return vl_fail(v, PGRC_E_PARAM, "encode: at most three parts");
    if (out_cap && !out) return vl_fail(v, PGRC_E_PARAM, "encode: out is NULL");
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_parts; k++) {
        if (parts[k].len && !parts[k].ptr) return vl_fail(v, PGRC_E_PARAM, "encode: part " + std::to_string(k) + " is NULL");
        if (n + parts[k].len < n) return vl_fail(v, PGRC_E_PARAM, "encode: the parts' lengths overflow");
        n += parts[k].len;
    }
    PGRC_ON_DEVICE(v);
    const auto t0 = std::chrono::steady_clock::now();
    v->tm = pgrc_varlen_times{};
    v->tm.symbols = n;
    if (!n) return PGRC_OK;
    for (uint32_t k = 0; k < n_parts; k++)
        if (parts[k].len && parts[k].on_device && !vl_is_device_ptr(parts[k].ptr))
            return vl_fail(v, PGRC_E_PARAM, "encode: part " + std::to_string(k) + " is flagged on_device but is no device pointer");
    if (out_cap && out_on_device && !vl_is_device_ptr(out)) return vl_fail(v, PGRC_E_PARAM, "encode: out is flagged on_device but is no device pointer");
    hipStream_t st = v->stream;
    int e;
    // the parts: host parts go up to their place in one joined buffer, device parts are read where they lie
    uint64_t host_bytes = 0;
    for (uint32_t k = 0; k < n_parts; k++)
        if (!parts[k].on_device) host_bytes += parts[k].len;
    if (host_bytes && (e = pgrc_buf_unpooled(v, v->d_src, n))) return e;
    VlSrc s{};
    s.n = n;
    uint64_t at = 0;
    for (uint32_t k = 0; k < 3; k++) {
        const uint64_t len = k < n_parts ? parts[k].len : 0;
        s.p[k] = nullptr;
        if (len) {
            if (parts[k].on_device) s.p[k] = (const uint8_t *)parts[k].ptr;
            else {
                s.p[k] = (const uint8_t *)v->d_src.p + at;
                HIP_TRY(v, hipMemcpyAsync((uint8_t *)v->d_src.p + at, parts[k].ptr, len, hipMemcpyHostToDevice, st));
            }
        }
        at += len;
        s.end[k] = at;
    }
    if (host_bytes) {
        HIP_TRY(v, hipStreamSynchronize(st));
        v->tm.ms_upload = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    const uint64_t nb = (n + VL_TILE - 1) / VL_TILE;
    if (nb > 0x7FFFFFFFull) return vl_fail(v, PGRC_E_PARAM, "encode: the text is too long");
    if ((e = pgrc_bufs_unpooled(v, {{&v->d_bmap, nb * 4}, {&v->d_bent, nb * 4}, {&v->d_bcnt, nb * 8}, {&v->d_bbase, (nb + 1) * 8}, {&v->d_fold, sco_scratch_elems(nb) * 8}})))
        return e;
    uint32_t *bmap = (uint32_t *)v->d_bmap.p, *bent = (uint32_t *)v->d_bent.p, *d_bad = (uint32_t *)v->d_flag.p;
    uint64_t *bcnt = (uint64_t *)v->d_bcnt.p, *bbase = (uint64_t *)v->d_bbase.p;
    const VlTables *tab = (const VlTables *)v->d_tab.p;
    HIP_TRY(v, hipMemsetAsync(d_bad, 0, 4, st));
    HIP_TRY(v, v->ev.record(0, st));
    hipLaunchKernelGGL(k_vl_maps, dim3((uint32_t)nb), dim3(VL_TPB), 0, st, s, tab, bmap, bcnt, d_bad);
    HIP_TRY(v, hipGetLastError());
    HIP_TRY(v, v->ev.record(1, st));
    HIP_TRY(v, (sco_device_scan<false, false>(st, ScoLoad<uint32_t, uint32_t, ScoIdentity>{bmap, ScoIdentity{}}, nb, ScoMap4{}, (uint32_t)SCO_MAP4_IDENTITY,
                                             (uint32_t)SCO_MAP4_IDENTITY, ScoStore<uint32_t>{bent}, (uint32_t *)v->d_fold.p)));
    HIP_TRY(v, (sco_device_scan<false, true>(st, VlBlockCount{bcnt, bent}, nb, ScoPlus{}, (uint64_t)0, (uint64_t)0, ScoStore<uint64_t>{bbase},
                                            (uint64_t *)v->d_fold.p)));
    uint64_t total = 0;
    uint32_t bad = 0;
    HIP_TRY(v, hipMemcpyAsync(&total, bbase + nb, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(v, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(v, v->ev.record(2, st));
    HIP_TRY(v, hipStreamSynchronize(st));
    if (bad) return vl_fail(v, PGRC_E_SYMBOL, "encode: the text holds a byte that is no symbol of the book");
    if (total > n) return vl_fail(v, PGRC_E_DEVICE, "encode: inconsistent counts");
    *coded_len = total;
    v->tm.coded_bytes = total;
    if (total > out_cap) return vl_fail(v, PGRC_E_PARAM, "encode: out_cap " + std::to_string(out_cap) + " is below the coded length " + std::to_string(total));
    uint8_t *d_out = (uint8_t *)out;
    if (!out_on_device) {
        if ((e = pgrc_buf_unpooled(v, v->d_coded, total))) return e;
        d_out = (uint8_t *)v->d_coded.p;
    }
    hipLaunchKernelGGL(k_vl_emit, dim3((uint32_t)nb), dim3(VL_TPB), 0, st, s, tab, (const uint32_t *)bent, (const uint64_t *)bbase, d_out, total);
    HIP_TRY(v, hipGetLastError());
    HIP_TRY(v, v->ev.record(3, st));
    HIP_TRY(v, hipStreamSynchronize(st));
    if (!out_on_device) {
        const auto t1 = std::chrono::steady_clock::now();
        HIP_TRY(v, hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, st));
        HIP_TRY(v, hipStreamSynchronize(st));
        v->tm.ms_download = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count();
    }
    v->tm.ms_maps = v->ev.ms(0, 1);
    v->tm.ms_scan = v->ev.ms(1, 2);
    v->tm.ms_emit = v->ev.ms(2, 3);
    v->tm.ms_call = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PGRC_OK;
}

int pgrc_varlen_decode(pgrc_varlen *v, const void *coded, uint64_t coded_len, int32_t coded_on_device, uint64_t expected_len, void *out,
                       int32_t out_on_device) {
    if (!v) return PGRC_E_PARAM;
    if (coded_len && !coded) return vl_fail(v, PGRC_E_PARAM, "decode: coded is NULL");
    if (expected_len && !out) return vl_fail(v, PGRC_E_PARAM, "decode: out is NULL");
    PGRC_ON_DEVICE(v);
    const auto t0 = std::chrono::steady_clock::now();
    v->tm = pgrc_varlen_times{};
    v->tm.was_decode = 1;
    v->tm.coded_bytes = coded_len;
    const uint64_t m = coded_len;
    if (!m) {
        if (expected_len) return vl_fail(v, PGRC_E_PARAM, "decode: unexpected decoded length 0 (expected " + std::to_string(expected_len) + ")");
        return PGRC_OK;
    }
    if (coded_on_device && !vl_is_device_ptr(coded)) return vl_fail(v, PGRC_E_PARAM, "decode: coded is flagged on_device but is no device pointer");
    if (expected_len && out_on_device && !vl_is_device_ptr(out)) return vl_fail(v, PGRC_E_PARAM, "decode: out is flagged on_device but is no device pointer");
    hipStream_t st = v->stream;
    int e;
    const uint8_t *d_coded = (const uint8_t *)coded;
    if (!coded_on_device) {
        if ((e = pgrc_buf_unpooled(v, v->d_coded, m))) return e;
        HIP_TRY(v, hipMemcpyAsync(v->d_coded.p, coded, m, hipMemcpyHostToDevice, st));
        HIP_TRY(v, hipStreamSynchronize(st));
        d_coded = (const uint8_t *)v->d_coded.p;
        v->tm.ms_upload = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    const uint64_t nb = (m + VL_DTILE - 1) / VL_DTILE;
    if (nb > 0x7FFFFFFFull) return vl_fail(v, PGRC_E_PARAM, "decode: the coded stream is too long");
    if ((e = pgrc_bufs_unpooled(v, {{&v->d_bsum, nb * 4}, {&v->d_bbase, (nb + 1) * 8}, {&v->d_fold, sco_scratch_elems(nb) * 8}}))) return e;
    uint32_t *bsum = (uint32_t *)v->d_bsum.p;
    uint64_t *bbase = (uint64_t *)v->d_bbase.p;
    const VlBook *book = (const VlBook *)v->d_book.p;
    HIP_TRY(v, v->ev.record(0, st));
    hipLaunchKernelGGL(k_vl_declen, dim3((uint32_t)nb), dim3(VL_TPB), 0, st, d_coded, m, book, bsum);
    HIP_TRY(v, hipGetLastError());
    HIP_TRY(v, v->ev.record(1, st));
    HIP_TRY(v, (sco_sum_u64<false>(st, (const uint32_t *)bsum, nb, bbase, (uint64_t *)v->d_fold.p)));
    uint64_t total = 0;
    HIP_TRY(v, hipMemcpyAsync(&total, bbase + nb, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(v, v->ev.record(2, st));
    HIP_TRY(v, hipStreamSynchronize(st));
    v->tm.symbols = total;
    if (total != expected_len)
        return vl_fail(v, PGRC_E_PARAM, "decode: unexpected decoded length " + std::to_string(total) + " (expected " + std::to_string(expected_len) + ")");
    if (total) {
        uint8_t *d_out = (uint8_t *)out;
        if (!out_on_device) {
            if ((e = pgrc_buf_unpooled(v, v->d_text, total))) return e;
            d_out = (uint8_t *)v->d_text.p;
        }
        hipLaunchKernelGGL(k_vl_expand, dim3((uint32_t)nb), dim3(VL_TPB), 0, st, d_coded, m, book, (const uint64_t *)bbase, d_out, total);
        HIP_TRY(v, hipGetLastError());
        HIP_TRY(v, v->ev.record(3, st));
        HIP_TRY(v, hipStreamSynchronize(st));
        if (!out_on_device) {
            const auto t1 = std::chrono::steady_clock::now();
            HIP_TRY(v, hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, st));
            HIP_TRY(v, hipStreamSynchronize(st));
            v->tm.ms_download = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count();
        }
        v->tm.ms_emit = v->ev.ms(2, 3);
    }
    v->tm.ms_maps = v->ev.ms(0, 1);
    v->tm.ms_scan = v->ev.ms(1, 2);
    v->tm.ms_call = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PGRC_OK;
}

} // extern "C"
