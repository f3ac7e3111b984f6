// huf.hip -- the Huffman mode of the reference's coder type 5 on gfx950 (include/pgrc_huf.h; libpgrc_huf.so).
//
// Reference behaviour restated (not translated): FSECompress / FSEUncompress in HUF_MODE (coders/FSECoder.cpp:15-135) over
// HUF_compress2 / HUF_decompress (coders/fse/huf_compress.c, huf_decompress.c, entropy_common.c).  The format leaves the
// writer its choices; they are the ones tests/huf_util.py fixes, and every kernel here follows that file byte for byte
// (DESIGN.md 4.25).
//   encode   k_huf_tables   a block per chunk: a histogram per segment (a wave each, in LDS), the ranks of the symbols, the
//                           tree and the length limit (one lane, <= 255 steps), lengths, values and the bit totals of the four
//                           segments (all threads), the weight header (one lane), the verdict raw / RLE / coded
//            the scan       scanops.h over the chunks' coded sizes
//            k_huf_emit     a block per segment: tiles of 4096 symbols from the segment's end to its start; a thread takes 16
//                           consecutive symbols, a block scan gives its bit offset, the codes are gathered in registers and
//                           OR-ed into a window of zeroed LDS words; whole words go to the chunk's slot
//            k_huf_compact  a block per chunk: size, header, jump table and the four streams (or the raw chunk) to their
//                           place in the frame, in aligned words
//   decode   k_huf_walk     one thread walks the sizes (each one says where the next one is) and checks them
//            k_huf_decode   a wave per chunk, four chunks a block: one lane reads the header, the wave fills the table of
//                           2^tableLog cells in LDS, lanes 0 .. 3 decode the four streams
// Integer work on streams; no MFMA, no library kernel, plain vector stores.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>

#include "scanops.h"

#include "ctx.h"
#include "pgrc_huf.h"

#define HF_TPB 256
#define HF_RUN 16                       // symbols of a thread (emit)
#define HF_TILE (HF_TPB * HF_RUN)       // symbols of a tile
#define HF_WIN (HF_TILE * PGRC_HUF_TABLE_LOG_MAX / 32 + 4)   // words a tile's codes may touch
#define HF_HDR 128                      // bytes of a weight header at most
#define HF_READ_LOG 12                  // code lengths the reader takes
#define HF_FSE_LOG 6                    // table log of the weight header's FSE table (the writer's; the reader takes 5 and 6)
#define HF_SLOT_PAD 32                  // a chunk's slot: its length and the rounding of four streams to words

enum { HF_RAW = 0, HF_RLE = 1, HF_HUF = 2 };

// what went wrong in a decode: the first chunk that reports wins (code | chunk << 8)
enum {
    HF_OK = 0, HF_E_CUT_SIZE, HF_E_CHUNK_SIZE, HF_E_TRAILING, HF_E_HDR_CUT, HF_E_FSE_LOG, HF_E_FSE_RUN, HF_E_FSE_SYMBOL, HF_E_FSE_SUM,
    HF_E_FSE_SPREAD, HF_E_FSE_STREAM, HF_E_FSE_LONG, HF_E_WEIGHT, HF_E_WEIGHT_SUM, HF_E_TABLE_LOG, HF_E_ODD, HF_E_JUMP, HF_E_NO_MARK,
    HF_E_STREAM_END, HF_E_COUNT
};
static const char *const HF_MESSAGES[HF_E_COUNT] = {
    "", "the frame ends inside a chunk's size", "a chunk's coded size is 0, above the chunk's length or past the frame's end",
    "bytes behind the last chunk", "weight header: cut short", "weight header: FSE table log above 6", "weight header: zero run past the last symbol",
    "weight header: a share for a weight above 11", "weight header: the FSE table's counts do not add up or run past the header",
    "weight header: the FSE table's counts do not fill the table", "weight header: no FSE stream, or one shorter than its two states",
    "weight header: more than 255 weights", "weight header: a weight above 11", "weight header: the weights' sum leaves no power of two for the last symbol",
    "weight header: no weight, or a table log above 12", "weight header: an odd number of longest codes, or fewer than two",
    "jump table: no room for it and four streams, or the segments' sizes exceed the chunk", "a stream without its end mark",
    "a stream ends early or late"};

struct HufChunk {
    uint32_t kind, csize, hsize, rle;
    uint32_t segbytes[4];
};

struct pgrc_huf : PgrcDev {
    PhaseEvents<5> ev;
    DevBuf d_src, d_coded, d_text, d_out, d_meta, d_codes, d_hdr, d_sizes, d_off, d_fold, d_slot, d_flag;
    pgrc_huf_times tm{};
    DevBufList bufs() { return {&d_src, &d_coded, &d_text, &d_out, &d_meta, &d_codes, &d_hdr, &d_sizes, &d_off, &d_fold, &d_slot, &d_flag}; }
};

// ------------------------------------------------------------------------------------------------ device side
__host__ __device__ __forceinline__ uint32_t hf_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ uint32_t hf_highbit(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }     // x != 0
__device__ __forceinline__ uint64_t hf_chunk_len(uint64_t n, uint32_t order, uint64_t chunk) {
    const uint64_t at = chunk << order;
    return n - at < (1ull << order) ? n - at : (1ull << order);
}

// f(byte, times) for every byte of p[0, len), by the lanes of one wave: 16-byte loads where the address allows (each holds
// bytes of the range only), single bytes at both ends
template <typename F>
__device__ __forceinline__ void hf_wave_bytes(const uint8_t *p, uint32_t len, uint32_t lane, F f) {
    const uint32_t head = hf_min(len, (uint32_t)((16u - ((uintptr_t)p & 15u)) & 15u));
    if (lane < head) f(p[lane], 1u);
    const uint4 *q = reinterpret_cast<const uint4 *>(p + head);
    const uint32_t nq = (len - head) >> 4;
    for (uint32_t i = lane; i < nq; i += 64) {
        const uint4 v = q[i];
        const uint32_t b0 = v.x & 0xFFu;
        if (v.x == b0 * 0x01010101u && v.y == v.x && v.z == v.x && v.w == v.x) {     // a run of one symbol: one update
            f(b0, 16u);
        } else {
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 16; j++) f((w[j >> 2] >> (8 * (j & 3))) & 0xFFu, 1u);
        }
    }
    const uint32_t tail = head + (nq << 4);
    if (tail + lane < len) f(p[tail + lane], 1u);
}

// dst[0, len) = src[0, len) by `nthr` threads, this one being `t`: aligned words of dst, each made of the one or two aligned
// words of src that hold its bytes (so no load leaves the words that hold bytes of the range); single bytes at both ends
__device__ __forceinline__ void hf_copy(uint8_t *dst, const uint8_t *src, uint32_t len, uint32_t t, uint32_t nthr) {
    const uint32_t head = hf_min(len, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
    if (t < head) dst[t] = src[t];
    const uint32_t nw = (len - head) >> 2;
    uint32_t *d = reinterpret_cast<uint32_t *>(dst + head);
    const uintptr_t s0 = (uintptr_t)(src + head);
    const uint32_t sh = (uint32_t)(s0 & 3u) * 8u;
    const uint32_t *a = reinterpret_cast<const uint32_t *>(s0 & ~(uintptr_t)3);
    for (uint32_t i = t; i < nw; i += nthr) {
        const uint32_t lo = a[i];
        d[i] = sh ? (lo >> sh) | (a[i + 1] << (32u - sh)) : lo;
    }
    const uint32_t tail = head + (nw << 2);
    if (tail + t < len) dst[tail + t] = src[tail + t];
}

// bits added from bit 0 of byte 0 upwards into a byte buffer of `cap` bytes; bytes beyond it are counted, not written
struct HfBitsUp {
    uint8_t *buf;
    uint32_t cap, bytes = 0, nacc = 0;
    uint64_t acc = 0;
    __host__ __device__ HfBitsUp(uint8_t *b, uint32_t c) : buf(b), cap(c) {}
    __host__ __device__ void add(uint32_t value, uint32_t nbits) {
        acc |= (uint64_t)(value & ((1u << nbits) - 1u)) << nacc;
        nacc += nbits;
        while (nacc >= 8) {
            if (bytes < cap) buf[bytes] = (uint8_t)acc;
            bytes++;
            acc >>= 8;
            nacc -= 8;
        }
    }
    __host__ __device__ uint32_t close() {
        if (nacc) {
            if (bytes < cap) buf[bytes] = (uint8_t)acc;
            bytes++;
            acc = 0;
            nacc = 0;
        }
        return bytes;
    }
};

// nbits <= 16 bits from bit `pos` upwards of p[0, len), zero beyond
__host__ __device__ __forceinline__ uint32_t hf_bits_at(const uint8_t *p, uint32_t len, uint32_t pos, uint32_t nbits) {
    const uint32_t b = pos >> 3;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) v |= (b + j < len ? (uint32_t)p[b + j] : 0u) << (8 * j);
    return (v >> (pos & 7u)) & ((1u << nbits) - 1u);
}

// FSE_buildDTable's layout (fse_decompress.c:85-123) by one thread: norm[12] (-1: one cell at the top) -> the cells' symbol,
// bits and base.  false: the counts do not fill the table
__host__ __device__ inline bool hf_fse_spread(const int32_t *norm, uint32_t tl, uint8_t *sym, uint8_t *nb, uint8_t *base) {
    const uint32_t size = 1u << tl;
    uint32_t high = size - 1, nxt[12];
    for (uint32_t s = 0; s < 12; s++) {
        if (norm[s] == -1) sym[high--] = (uint8_t)s;
        nxt[s] = norm[s] == -1 ? 1u : (uint32_t)norm[s];
    }
    const uint32_t step = (size >> 1) + (size >> 3) + 3;
    uint32_t pos = 0;
    for (uint32_t s = 0; s < 12; s++)
        for (int32_t i = 0; i < norm[s]; i++) {
            sym[pos] = (uint8_t)s;
            pos = (pos + step) & (size - 1);
            for (uint32_t guard = 0; pos > high && guard < size; guard++) pos = (pos + step) & (size - 1);
        }
    if (pos) return false;
    for (uint32_t u = 0; u < size; u++) {
        const uint32_t x = nxt[sym[u]]++;
        const uint32_t b = tl - hf_highbit(x);
        nb[u] = (uint8_t)b;
        base[u] = (uint8_t)((x << b) - size);
    }
    return true;
}

// ---- encode: tables
struct HfTabShared {
    uint32_t hist[4][256];
    uint32_t cnt[256];
    uint32_t node_w[256];
    uint16_t node_parent[256], leaf_parent[256];
    uint8_t order[256], lens[256], depth[256], weights[256];
    uint32_t bl[16], cum[16], start[16], segbits[4];
    uint32_t max_sym, max_len, rle, hsize;
    uint8_t fsym[64], fnb[64], fbase[64], pred[12][64], first[12];
    int32_t norm[12];
    uint8_t hdr[256];
};

// the weight header's FSE form into sh.hdr[1 ..]; -> its bytes (may exceed what fits).  Thread 0; sh.pred / sh.first made
// by all threads between the two parts
__host__ __device__ inline void hf_fse_norm(HfTabShared &sh, uint32_t nw) {
    uint32_t cnt[12] = {};
    for (uint32_t i = 0; i < nw; i++) cnt[sh.weights[i]]++;
    const int32_t size = 1 << HF_FSE_LOG;
    int32_t sum = 0, present = 0;
    for (uint32_t s = 0; s < 12; s++) {
        int32_t v = 0;
        if (cnt[s]) {
            v = (int32_t)(cnt[s] * (uint32_t)size / nw);
            if (v < 1) v = 1;
            present++;
        }
        sh.norm[s] = v;
    }
    if (present == 1) sh.norm[cnt[0] ? 1 : 0] = 1;
    for (uint32_t s = 0; s < 12; s++) sum += sh.norm[s];
    while (sum != size) {
        uint32_t k = 0;
        for (uint32_t s = 1; s < 12; s++)
            if (sh.norm[s] > sh.norm[k]) k = s;
        const int32_t d = sum < size ? 1 : -1;
        sh.norm[k] += d;
        sum += d;
    }
}

__host__ __device__ inline uint32_t hf_fse_write(HfTabShared &sh, uint32_t nw) {
    HfBitsUp b(sh.hdr + 1, sizeof sh.hdr - 1);
    b.add(HF_FSE_LOG - 5, 4);
    int32_t remaining = (1 << HF_FSE_LOG) + 1, threshold = 1 << HF_FSE_LOG;
    uint32_t nbits = HF_FSE_LOG + 1, s = 0;
    bool prev0 = false;
    while (remaining > 1 && s < 12) {
        if (prev0) {
            uint32_t run = 0;
            while (s + run < 11 && sh.norm[s + run] == 0) run++;
            s += run;
            while (run >= 3) { b.add(3, 2); run -= 3; }
            b.add(run, 2);
        }
        const int32_t c = sh.norm[s++];
        const int32_t v = c + 1, mx = 2 * threshold - 1 - remaining;
        if (v < mx) b.add((uint32_t)v, nbits - 1);
        else if (v < threshold) b.add((uint32_t)v, nbits);
        else b.add((uint32_t)(v + mx), nbits);
        remaining -= c;
        prev0 = c == 0;
        while (remaining < threshold) { nbits--; threshold >>= 1; }
    }
    const uint32_t head = b.close();
    const uint32_t room = (uint32_t)sizeof sh.hdr - 1u, used = hf_min(head, room);
    HfBitsUp o(sh.hdr + 1 + used, room - used);
    uint32_t st[2] = {0xFFu, 0xFFu};
    for (int32_t i = (int32_t)nw - 1; i >= 0; i--) {
        const uint32_t w = sh.weights[i], cur = st[i & 1];
        if (cur == 0xFFu) { st[i & 1] = sh.first[w]; continue; }
        const uint32_t u = sh.pred[w][cur];
        o.add(cur - sh.fbase[u], sh.fnb[u]);
        st[i & 1] = u;
    }
    o.add(st[1], HF_FSE_LOG);
    o.add(st[0], HF_FSE_LOG);
    o.add(1, 1);
    return head + o.close();
}

// the tree, the limit and the first code value of every length, by one thread: sh.cnt / sh.order of m >= 2 symbols -> sh.cum,
// sh.start, sh.max_len (tests/huf_util.py code_lengths)
__host__ __device__ inline void hf_tree(HfTabShared &sh, uint32_t m, uint32_t table_log) {
    // the tree: two queues, the leaves from the last rank on, the lighter head first, the leaf where both weigh the same
    int32_t leaf = (int32_t)m - 1;
    uint32_t head = 0;
    for (uint32_t k = 0; k + 1 < m; k++) {
        uint32_t w = 0;
        for (int two = 0; two < 2; two++) {
            if (leaf >= 0 && (head >= k || sh.cnt[sh.order[leaf]] <= sh.node_w[head])) {
                sh.leaf_parent[leaf] = (uint16_t)k;
                w += sh.cnt[sh.order[leaf]];
                leaf--;
            } else {
                sh.node_parent[head] = (uint16_t)k;
                w += sh.node_w[head];
                head++;
            }
        }
        sh.node_w[k] = w;
    }
    sh.depth[m - 2] = 0;
    for (int32_t k = (int32_t)m - 3; k >= 0; k--) {
        const uint32_t d = sh.depth[sh.node_parent[k]] + 1u;
        sh.depth[k] = (uint8_t)(d < 255u ? d : 255u);
    }
    for (uint32_t i = 0; i < 16; i++) sh.bl[i] = 0;
    for (uint32_t i = 0; i < m; i++) sh.bl[hf_min(sh.depth[sh.leaf_parent[i]] + 1u, table_log)]++;
    // the limit
    uint32_t total = 0;
    for (uint32_t i = 1; i <= table_log; i++) total += sh.bl[i] << (table_log - i);
    while (total > (1u << table_log)) {
        sh.bl[table_log]--;
        for (uint32_t i = table_log - 1; i > 0; i--)
            if (sh.bl[i]) {
                sh.bl[i]--;
                sh.bl[i + 1] += 2;
                break;
            }
        total--;
    }
    uint32_t cum = 0, mx = 1;
    for (uint32_t i = 1; i <= table_log; i++) {
        cum += sh.bl[i];
        sh.cum[i] = cum;
        if (sh.bl[i]) mx = i;
    }
    sh.max_len = mx;
    uint32_t low = 0;
    for (uint32_t i = mx; i > 0; i--) {
        sh.start[i] = low;
        low = (low + sh.bl[i]) >> 1;
    }
}

__global__ void __launch_bounds__(HF_TPB) k_huf_tables(const uint8_t *__restrict__ src, uint64_t n, uint32_t order, uint32_t table_log, uint64_t nch,
                                                       HufChunk *__restrict__ meta, uint32_t *__restrict__ codes, uint8_t *__restrict__ hdrs,
                                                       uint32_t *__restrict__ sizes, uint32_t *__restrict__ kinds) {
    __shared__ HfTabShared sh;
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint64_t chunk = blockIdx.x;
    const uint32_t len = (uint32_t)hf_chunk_len(n, order, chunk), seg = (len + 3) >> 2;
    const uint8_t *p = src + (chunk << order);
    for (uint32_t k = 0; k < 4; k++) sh.hist[k][t] = 0;
    if (t < 4) sh.segbits[t] = 0;
    if (t == 0) { sh.max_sym = 0; sh.rle = 0; sh.hsize = 0; }
    __syncthreads();
    {
        const uint32_t lo = hf_min(wv * seg, len), end = wv == 3 ? len : hf_min(lo + seg, len);
        uint32_t *hw = sh.hist[wv];
        hf_wave_bytes(p + lo, end - lo, lane, [&](uint32_t byte, uint32_t times) { atomicAdd(&hw[byte], times); });
    }
    __syncthreads();
    const uint32_t c = sh.hist[0][t] + sh.hist[1][t] + sh.hist[2][t] + sh.hist[3][t];
    sh.cnt[t] = c;
    sh.lens[t] = 0;
    if (c) atomicMax(&sh.max_sym, t);
    if (c == len) sh.rle = t;
    const uint32_t m = (uint32_t)__syncthreads_count(c != 0);
    uint32_t kind = HF_HUF;
    if (m == 1) kind = HF_RLE;
    else if (len < 12) kind = HF_RAW;
    if (kind == HF_HUF) {                                   // (block-uniform)
        // the ranks: falling count, equal counts by rising symbol
        if (c) {
            uint32_t rank = 0;
            for (uint32_t s = 0; s < 256; s++) {
                const uint32_t cs = sh.cnt[s];
                rank += (cs > c || (cs == c && s < t)) ? 1u : 0u;
            }
            sh.order[rank] = (uint8_t)t;
        }
        __syncthreads();
        if (t == 0) hf_tree(sh, m, table_log);
        __syncthreads();
        if (t < m) {                                        // rank t
            uint32_t ln = 1;
            while (ln < table_log && sh.cum[ln] <= t) ln++;
            sh.lens[sh.order[t]] = (uint8_t)ln;
        }
        __syncthreads();
        const uint32_t ln = sh.lens[t], max_len = sh.max_len, max_sym = sh.max_sym;
        uint32_t val = 0;
        if (ln) {
            val = sh.start[ln];
            for (uint32_t s = 0; s < t; s++) val += sh.lens[s] == ln ? 1u : 0u;
        }
        codes[chunk * 256 + t] = val | ln << 16;
        sh.weights[t] = ln ? (uint8_t)(max_len + 1 - ln) : 0;
        for (uint32_t k = 0; k < 4; k++)
            if (sh.hist[k][t]) atomicAdd(&sh.segbits[k], sh.hist[k][t] * ln);
        __syncthreads();
        // the header
        if (max_sym <= 128) {
            if (t == 0) sh.hdr[0] = (uint8_t)(127 + max_sym);
            if (2 * t < max_sym) sh.hdr[1 + t] = (uint8_t)(sh.weights[2 * t] << 4 | (2 * t + 1 < max_sym ? sh.weights[2 * t + 1] : 0));
            if (t == 0) sh.hsize = 1 + (max_sym + 1) / 2;
            __syncthreads();
        } else {
            if (t == 0) {
                hf_fse_norm(sh, max_sym);
                (void)hf_fse_spread(sh.norm, HF_FSE_LOG, sh.fsym, sh.fnb, sh.fbase);
            }
            __syncthreads();
            for (uint32_t i = t; i < 12 * 64; i += HF_TPB) {     // the cell of weight w whose interval holds state cur
                const uint32_t w = i >> 6, cur = i & 63;
                uint32_t found = 0;
                for (uint32_t u = 0; u < 64; u++)
                    if (sh.fsym[u] == w && sh.fbase[u] <= cur && cur < sh.fbase[u] + (1u << sh.fnb[u])) found = u;
                sh.pred[w][cur] = (uint8_t)found;
            }
            if (t < 12) {
                uint32_t f = 0;
                for (int32_t u = 63; u >= 0; u--)
                    if (sh.fsym[u] == t) f = (uint32_t)u;
                sh.first[t] = (uint8_t)f;
            }
            __syncthreads();
            if (t == 0) {
                const uint32_t body = hf_fse_write(sh, max_sym);
                sh.hdr[0] = (uint8_t)body;
                sh.hsize = body <= 127 ? 1 + body : 0;       // 0: no header fits, the chunk is stored raw
            }
            __syncthreads();
        }
        const uint32_t hsize = sh.hsize;
        if (t < hsize && t < HF_HDR) hdrs[chunk * HF_HDR + t] = sh.hdr[t];
        const uint32_t csize = hsize + 6 + (sh.segbits[0] + 8) / 8 + (sh.segbits[1] + 8) / 8 + (sh.segbits[2] + 8) / 8 + (sh.segbits[3] + 8) / 8;
        if (!hsize || csize >= len) kind = HF_RAW;
        if (t == 0 && kind == HF_HUF) {
            HufChunk mc;
            mc.kind = HF_HUF; mc.csize = csize; mc.hsize = hsize; mc.rle = 0;
            for (uint32_t k = 0; k < 4; k++) mc.segbytes[k] = (sh.segbits[k] + 8) / 8;
            meta[chunk] = mc;
            sizes[chunk] = csize + (chunk + 1 < nch ? 4u : 0u);
            atomicAdd(&kinds[HF_HUF], 1u);
        }
    }
    if (t == 0 && kind != HF_HUF) {
        HufChunk mc{};
        mc.kind = kind;
        mc.csize = kind == HF_RLE ? 1u : len;
        mc.rle = sh.rle;
        meta[chunk] = mc;
        sizes[chunk] = mc.csize + (chunk + 1 < nch ? 4u : 0u);
        atomicAdd(&kinds[kind], 1u);
    }
}

// a chunk's slot: four streams, each from a word boundary on
__device__ __forceinline__ uint32_t hf_slot_off(const HufChunk &mc, uint32_t k) {
    uint32_t o = 0;
    for (uint32_t j = 0; j < k; j++) o += (mc.segbytes[j] + 3u) & ~3u;
    return o;
}

// ---- encode: the streams.  blockIdx.x: the segment, blockIdx.y: the chunk
__global__ void __launch_bounds__(HF_TPB) k_huf_emit(const uint8_t *__restrict__ src, uint64_t n, uint32_t order, const HufChunk *__restrict__ meta,
                                                     const uint32_t *__restrict__ codes, uint8_t *__restrict__ slots, uint64_t slot_stride) {
    __shared__ uint32_t code[256];
    __shared__ uint32_t win[HF_WIN];
    __shared__ uint32_t sm32[HF_TPB / 64];
    const uint64_t chunk = blockIdx.y;
    const uint32_t k = blockIdx.x, t = threadIdx.x;
    const HufChunk mc = meta[chunk];
    if (mc.kind != HF_HUF) return;                          // (block-uniform)
    const uint32_t len = (uint32_t)hf_chunk_len(n, order, chunk), seg = (len + 3) >> 2;
    const uint32_t lo = k * seg, hi = k == 3 ? len : lo + seg;          // (len >= 12: 3 * seg < len)
    const uint8_t *p = src + (chunk << order);
    uint32_t *out = reinterpret_cast<uint32_t *>(slots + chunk * slot_stride + hf_slot_off(mc, k));
    const uint32_t out_words = (mc.segbytes[k] + 3u) >> 2;
    code[t] = codes[chunk * 256 + t];
    uint32_t base = 0, carry = 0;                           // bits written so far; the bits of the word they end in
    for (uint32_t te = hi; te > lo; te -= hf_min(te - lo, HF_TILE)) {
        for (uint32_t i = t; i < HF_WIN; i += HF_TPB) win[i] = 0;
        __syncthreads();
        // the thread's run: symbols [r0, r1) of the chunk, thread 0 the tile's last ones
        const uint32_t tb = te - hf_min(te - lo, HF_TILE);
        const uint32_t r1 = te > t * HF_RUN ? te - t * HF_RUN : 0;
        const uint32_t r1c = r1 > tb ? r1 : tb, r0 = r1c - tb > HF_RUN ? r1c - HF_RUN : tb;
        uint32_t sym[HF_RUN / 4] = {};
        if (r1c - r0 == HF_RUN) {
            const uintptr_t a = (uintptr_t)(p + r0);
            const uint4 *q = reinterpret_cast<const uint4 *>(a & ~(uintptr_t)15);
            const uint32_t shb = (uint32_t)(a & 15u);
            const uint4 q0 = q[0];
            uint4 q1 = make_uint4(0, 0, 0, 0);
            if (shb) q1 = q[1];
            const uint32_t d[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t v = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const uint32_t at = shb + 4 * j + b;
                    v |= ((d[at >> 2] >> (8 * (at & 3))) & 0xFFu) << (8 * b);
                }
                sym[j] = v;
            }
        } else {
            for (uint32_t i = r0; i < r1c; i++) sym[(i - r0) >> 2] |= (uint32_t)p[i] << (8 * ((i - r0) & 3));
        }
        const uint32_t cnt = r1c - r0;
        uint32_t bits = 0;
#pragma unroll
        for (uint32_t i = 0; i < HF_RUN; i++)
            if (i < cnt) bits += code[(sym[i >> 2] >> (8 * (i & 3))) & 0xFFu] >> 16;
        uint32_t tilebits;
        const uint32_t off = sco_block_sum<HF_TPB / 64>(bits, sm32, &tilebits);
        // the run's codes from its last symbol up, gathered in a 64-bit register, whole words OR-ed into the window
        const uint32_t w0 = base >> 5;
        uint32_t rel = (base & 31u) + off, word = rel >> 5;
        uint64_t acc = 0;
        if (t == 0) acc = carry;                            // (thread 0's run starts at `base`: the word's lower bits are the carry)
#pragma unroll
        for (int i = HF_RUN - 1; i >= 0; i--) {
            if ((uint32_t)i < cnt) {
                const uint32_t c = code[(sym[i >> 2] >> (8 * (i & 3))) & 0xFFu];
                acc |= (uint64_t)(c & 0xFFFFu) << (rel - 32u * word);
                rel += c >> 16;
                if (rel - 32u * word >= 32u) {
                    if (word < HF_WIN) atomicOr(&win[word], (uint32_t)acc);
                    acc >>= 32;
                    word++;
                }
            }
        }
        if (acc && word < HF_WIN) atomicOr(&win[word], (uint32_t)acc);
        __syncthreads();
        const uint32_t nbase = base + tilebits, full = (nbase >> 5) - w0;
        for (uint32_t i = t; i < full && i < HF_WIN; i += HF_TPB)
            if (w0 + i < out_words) out[w0 + i] = win[i];
        carry = full < HF_WIN ? win[full] : 0;
        base = nbase;
        __syncthreads();
    }
    if (t == 0 && (base >> 5) < out_words) out[base >> 5] = carry | 1u << (base & 31u);     // the end mark
}

// ---- encode: compaction
__global__ void __launch_bounds__(HF_TPB) k_huf_compact(const uint8_t *__restrict__ src, uint64_t n, uint32_t order, uint32_t table_log, uint64_t nch,
                                                        const HufChunk *__restrict__ meta, const uint8_t *__restrict__ hdrs,
                                                        const uint8_t *__restrict__ slots, uint64_t slot_stride, const uint64_t *__restrict__ off,
                                                        uint8_t *__restrict__ out, uint64_t total) {
    const uint64_t chunk = blockIdx.x;
    const uint32_t t = threadIdx.x;
    const HufChunk mc = meta[chunk];
    const uint32_t len = (uint32_t)hf_chunk_len(n, order, chunk);
    const uint32_t pre = chunk + 1 < nch ? 4u : 0u;
    const uint64_t at = 4 + off[chunk];
    if (at + pre + mc.csize > total) return;                // (the sizes the scan saw; a source that changed in between stays inside)
    if (chunk == 0 && t < 4) out[t] = t == 0 ? 0 : t == 1 ? (uint8_t)order : t == 2 ? 255 : (uint8_t)table_log;
    uint8_t *dst = out + at;
    if (t < pre) dst[t] = (uint8_t)(mc.csize >> (8 * t));
    dst += pre;
    if (mc.kind == HF_RLE) {
        if (t == 0) dst[0] = (uint8_t)mc.rle;
    } else if (mc.kind == HF_RAW) {
        hf_copy(dst, src + (chunk << order), len, t, HF_TPB);
    } else {
        if (t < mc.hsize) dst[t] = hdrs[chunk * HF_HDR + t];
        dst += mc.hsize;
        if (t < 6) dst[t] = (uint8_t)(mc.segbytes[t >> 1] >> (8 * (t & 1)));
        dst += 6;
        const uint8_t *slot = slots + chunk * slot_stride;
        for (uint32_t k = 0; k < 4; k++) {
            hf_copy(dst, slot + hf_slot_off(mc, k), mc.segbytes[k], t, HF_TPB);
            dst += mc.segbytes[k];
        }
    }
}

// ---- decode
__device__ __forceinline__ void hf_report(uint32_t *err, uint32_t code, uint64_t chunk) {
    atomicCAS(err, 0u, code | (uint32_t)(chunk < 0xFFFFFFull ? chunk : 0xFFFFFFull) << 8);
}

// one thread: where every chunk's bytes are and how many (FSEUncompress's walk, FSECoder.cpp:100-132)
__global__ void k_huf_walk(const uint8_t *__restrict__ coded, uint64_t coded_len, uint64_t n, uint32_t order, uint64_t nch, uint64_t *__restrict__ at_out,
                           uint32_t *__restrict__ size_out, uint32_t *err) {
    uint64_t at = 4;
    for (uint64_t chunk = 0; chunk < nch; chunk++) {
        const uint64_t len = hf_chunk_len(n, order, chunk);
        uint64_t size;
        if (chunk + 1 < nch) {
            if (at + 4 > coded_len) { hf_report(err, HF_E_CUT_SIZE, chunk); return; }
            size = (uint64_t)coded[at] | (uint64_t)coded[at + 1] << 8 | (uint64_t)coded[at + 2] << 16 | (uint64_t)coded[at + 3] << 24;
            at += 4;
        } else {
            size = coded_len - at;
        }
        if (size < 1 || size > len || size > coded_len - at) { hf_report(err, HF_E_CHUNK_SIZE, chunk); return; }
        at_out[chunk] = at;
        size_out[chunk] = (uint32_t)size;
        at += size;
    }
    if (at != coded_len) hf_report(err, HF_E_TRAILING, nch - 1);
}

struct HfDecShared {
    uint16_t dt[1 << HF_READ_LOG];      // symbol | bits << 8
    uint8_t weights[256];
    uint16_t start[256];
    uint8_t fsym[64], fnb[64], fbase[64];
    uint32_t nsym, tl, ok, used;
    uint32_t seg_at[4], seg_len[4];
};

// HUF_readStats (entropy_common.c:154-215) by one lane: c[0, csize) -> d.weights / d.nsym / d.tl / d.used; 0 or what is wrong
__host__ __device__ inline uint32_t hf_read_stats(const uint8_t *c, uint32_t csize, HfDecShared &d) {
    const uint32_t h = c[0];
    uint32_t nw;
    if (h >= 128) {
        nw = h - 127;
        d.used = 1 + (nw + 1) / 2;
        if (d.used > csize) return HF_E_HDR_CUT;
        for (uint32_t i = 0; i < nw; i++) d.weights[i] = (i & 1) ? c[1 + (i >> 1)] & 15u : c[1 + (i >> 1)] >> 4;
    } else {
        d.used = 1 + h;
        if (d.used > csize || h < 2) return HF_E_HDR_CUT;
        const uint8_t *p = c + 1;
        // FSE_readNCount (entropy_common.c:40-144) as a plain bit stream
        uint32_t pos = 4;
        const uint32_t tl = hf_bits_at(p, h, 0, 4) + 5;
        if (tl > 6) return HF_E_FSE_LOG;
        int32_t remaining = (1 << tl) + 1, threshold = 1 << tl, norm[12] = {};
        uint32_t nbits = tl + 1, s = 0;
        bool prev0 = false;
        while (remaining > 1 && s <= 255) {
            if (prev0) {
                while (hf_bits_at(p, h, pos, 16) == 0xFFFFu && pos <= 8 * h) { s += 24; pos += 16; }
                while (hf_bits_at(p, h, pos, 2) == 3u && pos <= 8 * h) { s += 3; pos += 2; }
                s += hf_bits_at(p, h, pos, 2);
                pos += 2;
                if (s > 255) return HF_E_FSE_RUN;
            }
            const int32_t mx = 2 * threshold - 1 - remaining;
            int32_t cnt = (int32_t)hf_bits_at(p, h, pos, nbits - 1);
            if (cnt < mx) {
                pos += nbits - 1;
            } else {
                cnt = (int32_t)hf_bits_at(p, h, pos, nbits);
                if (cnt >= threshold) cnt -= mx;
                pos += nbits;
            }
            cnt--;
            remaining -= cnt < 0 ? -cnt : cnt;
            if (cnt && s >= 12) return HF_E_FSE_SYMBOL;
            if (s < 12) norm[s] = cnt;
            s++;
            prev0 = cnt == 0;
            while (remaining < threshold) { nbits--; threshold >>= 1; }
            if (pos > 8 * h) return HF_E_FSE_SUM;
        }
        if (remaining != 1) return HF_E_FSE_SUM;
        if (!hf_fse_spread(norm, tl, d.fsym, d.fnb, d.fbase)) return HF_E_FSE_SPREAD;
        // the two-state stream (fse_decompress.c:178-238), read from its end mark down
        const uint32_t nc = (pos + 7) >> 3;
        if (nc >= h || !p[h - 1]) return HF_E_FSE_STREAM;
        const uint8_t *q = p + nc;
        const uint32_t qlen = h - nc;
        int32_t left = (int32_t)(8 * (qlen - 1) + hf_highbit(q[qlen - 1]));
        if (left < (int32_t)(2 * tl)) return HF_E_FSE_STREAM;
        uint32_t st[2];
        for (int j = 0; j < 2; j++) {
            left -= (int32_t)tl;
            st[j] = hf_bits_at(q, qlen, (uint32_t)left, tl);
        }
        nw = 0;
        for (uint32_t i = 0;; i++) {
            if (nw > 253) return HF_E_FSE_LONG;
            const uint32_t u = st[i & 1];
            d.weights[nw++] = d.fsym[u];
            if ((int32_t)d.fnb[u] > left) {
                d.weights[nw++] = d.fsym[st[(i + 1) & 1]];
                break;
            }
            left -= d.fnb[u];
            st[i & 1] = d.fbase[u] + hf_bits_at(q, qlen, (uint32_t)left, d.fnb[u]);
        }
    }
    uint32_t total = 0, rank[HF_READ_LOG + 1] = {};
    for (uint32_t i = 0; i < nw; i++) {
        const uint32_t w = d.weights[i];
        if (w >= 12) return HF_E_WEIGHT;
        rank[w]++;
        total += (1u << w) >> 1;
    }
    if (!total) return HF_E_TABLE_LOG;
    const uint32_t tl = hf_highbit(total) + 1;
    if (tl > HF_READ_LOG) return HF_E_TABLE_LOG;
    const uint32_t rest = (1u << tl) - total;
    if (rest & (rest - 1)) return HF_E_WEIGHT_SUM;
    const uint32_t last = hf_highbit(rest) + 1;
    d.weights[nw] = (uint8_t)last;
    rank[last]++;
    if (rank[1] < 2 || (rank[1] & 1)) return HF_E_ODD;
    d.nsym = nw + 1;
    d.tl = tl;
    // where every symbol's cells start: by rising weight, within a weight by rising symbol (huf_decompress.c:151-183)
    uint32_t next[HF_READ_LOG + 1], run = 0;
    for (uint32_t w = 1; w <= tl; w++) {
        next[w] = run;
        run += rank[w] << (w - 1);
    }
    for (uint32_t s = 0; s < d.nsym; s++) {
        const uint32_t w = d.weights[s];
        if (w) {
            d.start[s] = (uint16_t)next[w];
            next[w] += 1u << (w - 1);
        }
    }
    return HF_OK;
}

// the jump table behind the header (huf_decompress.c:269-303) by one lane -> d.seg_at / d.seg_len, every stream inside the
// chunk and with its end mark; 0 or what is wrong
__host__ __device__ inline uint32_t hf_read_jump(const uint8_t *c, uint32_t csize, uint32_t len, HfDecShared &d) {
    const uint32_t seg = (len + 3) >> 2, blen = csize - d.used;
    const uint8_t *b = c + d.used;
    if (blen < 10 || 3 * seg > len) return HF_E_JUMP;
    uint32_t at = 6;
    for (uint32_t k = 0; k < 3; k++) {
        d.seg_at[k] = d.used + at;
        d.seg_len[k] = (uint32_t)b[2 * k] | (uint32_t)b[2 * k + 1] << 8;
        at += d.seg_len[k];
    }
    if (at >= blen) return HF_E_JUMP;
    d.seg_at[3] = d.used + at;
    d.seg_len[3] = blen - at;
    for (uint32_t k = 0; k < 4; k++)
        if (!d.seg_len[k] || !c[d.seg_at[k] + d.seg_len[k] - 1]) return HF_E_NO_MARK;
    return HF_OK;
}

// the 8 bytes from byte `at` of s[0, len), zero beyond
__host__ __device__ __forceinline__ uint64_t hf_load8(const uint8_t *s, uint32_t len, uint32_t at) {
    uint64_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) v |= (uint64_t)(at + j < len ? s[at + j] : 0) << (8 * j);
    return v;
}

// one stream: `count` symbols from under the end mark of s[0, slen) (its last byte is not 0) down, to q; -> the bits left over
// (0: the stream ends where it must).  Every read is checked against slen, and a stream that runs dry decodes zeros
__host__ __device__ inline int32_t hf_decode_stream(const uint16_t *dt, uint32_t tl, const uint8_t *s, uint32_t slen, uint8_t *q, uint32_t count) {
    const uint32_t mask = (1u << tl) - 1u;
    int32_t left = (int32_t)(8 * (slen - 1) + hf_highbit(s[slen - 1]));     // (the last byte is not 0: checked above)
    int32_t wb = -1;
    uint64_t win = 0;
    uint32_t pack = 0;
    for (uint32_t i = 0; i < count; i++) {
        const int32_t p = left - (int32_t)tl;
        uint32_t v;
        if (p >= 0) {
            if (wb < 0 || p < 8 * wb || p + (int32_t)tl > 8 * wb + 64) {
                wb = ((p + (int32_t)tl + 7) >> 3) - 8;
                if (wb < 0) wb = 0;
                win = hf_load8(s, slen, (uint32_t)wb);
            }
            v = (uint32_t)(win >> (p - 8 * wb)) & mask;
        } else if (left > 0) {                          // fewer than tl bits are left: zeros stand below bit 0
            if (wb != 0) { wb = 0; win = hf_load8(s, slen, 0); }
            v = ((uint32_t)win & ((1u << left) - 1u)) << (tl - (uint32_t)left);
        } else {
            v = 0;
        }
        const uint32_t e = dt[v];
        left -= (int32_t)(e >> 8);
        // whole aligned words where the place allows, single bytes at both ends
        const uint32_t al = (uint32_t)((uintptr_t)(q + i) & 3u);
        pack |= (e & 0xFFu) << (8 * al);
        if (al == 3u || i + 1 == count) {
            const uint32_t nbytes = hf_min(al + 1, i + 1);       // gathered since the last word: they end at place `al`
            if (nbytes == 4) *reinterpret_cast<uint32_t *>(q + i - 3) = pack;
            else
                for (uint32_t j = 0; j < nbytes; j++) q[i - j] = (uint8_t)(pack >> (8 * (al - j)));
            pack = 0;
        }
    }
    return left;
}

__global__ void __launch_bounds__(HF_TPB) k_huf_decode(const uint8_t *__restrict__ coded, const uint64_t *__restrict__ at_in, const uint32_t *__restrict__ size_in,
                                                       uint64_t n, uint32_t order, uint64_t nch, uint8_t *__restrict__ out, uint32_t *err, uint32_t *__restrict__ kinds) {
    __shared__ HfDecShared sh[HF_TPB / 64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t chunk = (uint64_t)blockIdx.x * (HF_TPB / 64) + wv;
    HfDecShared &d = sh[wv];
    const bool live = chunk < nch;
    const uint32_t len = live ? (uint32_t)hf_chunk_len(n, order, chunk) : 0;
    const uint32_t csize = live ? size_in[chunk] : 0;
    const uint8_t *c = coded + (live ? at_in[chunk] : 0);
    uint8_t *o = out + (chunk << order);
    const bool huf = live && csize != len && csize != 1;
    if (lane == 0) {
        d.ok = 0;
        if (huf) {
            uint32_t e = hf_read_stats(c, csize, d);
            if (!e) e = hf_read_jump(c, csize, len, d);
            if (e) hf_report(err, e, chunk);
            d.ok = e ? 0u : 1u;
        }
        if (live) atomicAdd(&kinds[huf ? HF_HUF : csize == 1 && len != 1 ? HF_RLE : HF_RAW], 1u);
    }
    __syncthreads();
    if (live && !huf) {
        if (csize == len) hf_copy(o, c, len, lane, 64);
        else {
            const uint8_t b = c[0];
            for (uint32_t i = lane; i < len; i += 64) o[i] = b;
        }
    }
    const bool ok = huf && d.ok;
    if (ok) {
        const uint32_t tl = d.tl;
        for (uint32_t s = 0; s < d.nsym; s++) {
            const uint32_t w = d.weights[s];
            if (!w) continue;
            const uint32_t span = 1u << (w - 1), st = d.start[s];
            const uint16_t e = (uint16_t)(s | (tl + 1 - w) << 8);
            for (uint32_t u = lane; u < span; u += 64)
                if (st + u < (1u << HF_READ_LOG)) d.dt[st + u] = e;
        }
    }
    __syncthreads();
    if (ok && lane < 4) {
        const uint32_t tl = d.tl, seg = (len + 3) >> 2;
        const uint32_t first = lane * seg, count = lane == 3 ? len - 3 * seg : seg;
        const uint8_t *s = c + d.seg_at[lane];
        const uint32_t slen = d.seg_len[lane];
        const int32_t left = hf_decode_stream(d.dt, tl, s, slen, o + first, count);
        if (left != 0) hf_report(err, HF_E_STREAM_END, chunk);
    }
}

// ------------------------------------------------------------------------------------------------ host side
static thread_local std::string g_hf_create_err;

static int hf_fail(pgrc_huf *h, int code, const std::string &msg) {
    h->err = msg;
    return code;
}

static bool hf_is_device_ptr(const void *p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) == hipSuccess) return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
    (void)hipGetLastError();
    return false;
}

static uint64_t hf_chunks(uint64_t n, uint32_t order) { return (n + (1ull << order) - 1) >> order; }

extern "C" {

uint64_t pgrc_huf_bound(uint64_t n, uint32_t block_order) {
    if (block_order < 1 || block_order > PGRC_HUF_ORDER_MAX) return 0;
    const uint64_t nch = hf_chunks(n, block_order);
    return 4 + n + 4 * (nch ? nch - 1 : 0);
}

void pgrc_huf_destroy(pgrc_huf *h) {
    if (!h) return;
    PgrcDeviceScope scope(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    dec_free_all(h->bufs());
    h->ev.release();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

const char *pgrc_huf_last_error(const pgrc_huf *h) { return h ? h->err.c_str() : g_hf_create_err.c_str(); }

int pgrc_huf_create(int32_t device, pgrc_huf **out) {
    if (!out) return PGRC_E_PARAM;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        g_hf_create_err = "no HIP device";
        return PGRC_E_NO_DEVICE;
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess) { g_hf_create_err = "hipGetDevice failed"; return PGRC_E_NO_DEVICE; }
    if (device >= ndev) { g_hf_create_err = "device " + std::to_string(device) + " does not exist"; return PGRC_E_NO_DEVICE; }
    pgrc_huf *h = new pgrc_huf();
    h->device = device;
    PgrcDeviceScope scope(device);
    int e = scope.ok ? PGRC_OK : PGRC_E_NO_DEVICE;
    if (!e && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) e = PGRC_E_DEVICE;
    if (!e && h->ev.ensure(h)) e = PGRC_E_DEVICE;
    if (!e) e = pgrc_buf_unpooled(h, h->d_flag, 64);
    if (e) {
        g_hf_create_err = h->err.empty() ? "HIP stream / event creation failed" : h->err;
        (void)hipGetLastError();
        pgrc_huf_destroy(h);
        return e;
    }
    *out = h;
    return PGRC_OK;
}

int pgrc_huf_timing(pgrc_huf *h, pgrc_huf_times *out) {
    if (!h || !out) return PGRC_E_PARAM;
    *out = h->tm;
    return PGRC_OK;
}

int pgrc_huf_encode(pgrc_huf *h, const void *src, uint64_t n, int32_t src_on_device, uint32_t block_order, uint32_t table_log, void *out,
                    uint64_t out_cap, int32_t out_on_device, uint64_t *coded_len) {
    if (!h) return PGRC_E_PARAM;
    if (!coded_len) return hf_fail(h, PGRC_E_PARAM, "encode: coded_len is NULL");
    *coded_len = 0;
    if (n && !src) return hf_fail(h, PGRC_E_PARAM, "encode: src is NULL");
    if (out_cap && !out) return hf_fail(h, PGRC_E_PARAM, "encode: out is NULL");
    if (block_order < 1 || block_order > PGRC_HUF_ORDER_MAX) return hf_fail(h, PGRC_E_PARAM, "encode: block_order " + std::to_string(block_order) + " is outside 1 .. 17");
    if (!table_log) table_log = PGRC_HUF_TABLE_LOG_MAX;
    if (table_log < PGRC_HUF_TABLE_LOG_MIN || table_log > PGRC_HUF_TABLE_LOG_MAX)
        return hf_fail(h, PGRC_E_PARAM, "encode: table_log " + std::to_string(table_log) + " is outside 8 .. 11");
    const uint64_t nch = hf_chunks(n, block_order);
    if (nch > 0x7FFFFFFFull / 4) return hf_fail(h, PGRC_E_PARAM, "encode: too many chunks; use a larger block_order");
    PGRC_ON_DEVICE(h);
    const auto t0 = std::chrono::steady_clock::now();
    h->tm = pgrc_huf_times{};
    h->tm.bytes = n;
    h->tm.chunks = (uint32_t)nch;
    if (n && src_on_device && !hf_is_device_ptr(src)) return hf_fail(h, PGRC_E_PARAM, "encode: src is flagged on_device but is no device pointer");
    if (out_cap && out_on_device && !hf_is_device_ptr(out)) return hf_fail(h, PGRC_E_PARAM, "encode: out is flagged on_device but is no device pointer");
    hipStream_t st = h->stream;
    int e;
    if (!n) {
        *coded_len = 4;
        h->tm.coded_bytes = 4;
        if (out_cap < 4) return hf_fail(h, PGRC_E_PARAM, "encode: out_cap " + std::to_string(out_cap) + " is below the coded length 4");
        const uint8_t props[4] = {0, (uint8_t)block_order, 255, (uint8_t)table_log};
        if (out_on_device) {
            HIP_TRY(h, hipMemcpyAsync(out, props, 4, hipMemcpyHostToDevice, st));
            HIP_TRY(h, hipStreamSynchronize(st));
        } else {
            memcpy(out, props, 4);
        }
        return PGRC_OK;
    }
    const uint8_t *d_src = (const uint8_t *)src;
    if (!src_on_device) {
        if ((e = pgrc_buf_unpooled(h, h->d_src, n))) return e;
        HIP_TRY(h, hipMemcpyAsync(h->d_src.p, src, n, hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        d_src = (const uint8_t *)h->d_src.p;
        h->tm.ms_upload = dec_ms_since(t0);
    }
    const uint64_t slot_stride = (((1ull << block_order) + HF_SLOT_PAD) + 15) & ~15ull;
    if ((e = pgrc_bufs_unpooled(h, {{&h->d_meta, nch * sizeof(HufChunk)}, {&h->d_codes, nch * 1024}, {&h->d_hdr, nch * HF_HDR}, {&h->d_sizes, nch * 4},
                                    {&h->d_off, (nch + 1) * 8}, {&h->d_fold, sco_scratch_elems(nch) * 8}, {&h->d_slot, nch * slot_stride}})))
        return e;
    HufChunk *meta = (HufChunk *)h->d_meta.p;
    uint32_t *codes = (uint32_t *)h->d_codes.p, *sizes = (uint32_t *)h->d_sizes.p, *kinds = (uint32_t *)h->d_flag.p;
    uint8_t *hdrs = (uint8_t *)h->d_hdr.p, *slots = (uint8_t *)h->d_slot.p;
    uint64_t *off = (uint64_t *)h->d_off.p;
    HIP_TRY(h, hipMemsetAsync(kinds, 0, 64, st));
    HIP_TRY(h, h->ev.record(0, st));
    hipLaunchKernelGGL(k_huf_tables, dim3((uint32_t)nch), dim3(HF_TPB), 0, st, d_src, n, block_order, table_log, nch, meta, codes, hdrs, sizes, kinds);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, h->ev.record(1, st));
    HIP_TRY(h, (sco_sum_u64<false>(st, (const uint32_t *)sizes, nch, off, (uint64_t *)h->d_fold.p)));
    uint64_t total = 0;
    uint32_t hk[4] = {};
    HIP_TRY(h, hipMemcpyAsync(&total, off + nch, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(hk, kinds, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, h->ev.record(2, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    total += 4;
    if (total > pgrc_huf_bound(n, block_order)) return hf_fail(h, PGRC_E_DEVICE, "encode: inconsistent sizes");
    *coded_len = total;
    h->tm.coded_bytes = total;
    h->tm.raw_chunks = hk[HF_RAW];
    h->tm.rle_chunks = hk[HF_RLE];
    h->tm.huf_chunks = hk[HF_HUF];
    if (total > out_cap) return hf_fail(h, PGRC_E_PARAM, "encode: out_cap " + std::to_string(out_cap) + " is below the coded length " + std::to_string(total));
    uint8_t *d_out = (uint8_t *)out;
    if (!out_on_device) {
        if ((e = pgrc_buf_unpooled(h, h->d_out, total))) return e;
        d_out = (uint8_t *)h->d_out.p;
    }
    if (hk[HF_HUF]) {
        for (uint64_t c0 = 0; c0 < nch; c0 += 32768) {       // (a grid's second dimension ends at 65535)
            const uint32_t cn = (uint32_t)std::min<uint64_t>(nch - c0, 32768);
            hipLaunchKernelGGL(k_huf_emit, dim3(4, cn), dim3(HF_TPB), 0, st, d_src + (c0 << block_order), n - (c0 << block_order), block_order,
                               (const HufChunk *)meta + c0, (const uint32_t *)codes + c0 * 256, slots + c0 * slot_stride, slot_stride);
            HIP_TRY(h, hipGetLastError());
        }
    }
    HIP_TRY(h, h->ev.record(3, st));
    hipLaunchKernelGGL(k_huf_compact, dim3((uint32_t)nch), dim3(HF_TPB), 0, st, d_src, n, block_order, table_log, nch, (const HufChunk *)meta,
                       (const uint8_t *)hdrs, (const uint8_t *)slots, slot_stride, (const uint64_t *)off, d_out, total);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, h->ev.record(4, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (!out_on_device) {
        const auto t1 = std::chrono::steady_clock::now();
        HIP_TRY(h, hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        h->tm.ms_download = dec_ms_since(t1);
    }
    h->tm.ms_tables = h->ev.ms(0, 1);
    h->tm.ms_emit = h->ev.ms(2, 3);
    h->tm.ms_compact = h->ev.ms(1, 2) + h->ev.ms(3, 4);
    h->tm.ms_call = dec_ms_since(t0);
    return PGRC_OK;
}

int pgrc_huf_decode(pgrc_huf *h, const void *coded, uint64_t coded_len, int32_t coded_on_device, uint64_t expected_len, void *out,
                    int32_t out_on_device) {
    if (!h) return PGRC_E_PARAM;
    if (!coded) return hf_fail(h, PGRC_E_PARAM, "decode: coded is NULL");
    if (expected_len && !out) return hf_fail(h, PGRC_E_PARAM, "decode: out is NULL");
    if (coded_len < 4) return hf_fail(h, PGRC_E_PARAM, "decode: the frame is shorter than its four props bytes");
    PGRC_ON_DEVICE(h);
    const auto t0 = std::chrono::steady_clock::now();
    h->tm = pgrc_huf_times{};
    h->tm.was_decode = 1;
    h->tm.coded_bytes = coded_len;
    h->tm.bytes = expected_len;
    if (coded_on_device && !hf_is_device_ptr(coded)) return hf_fail(h, PGRC_E_PARAM, "decode: coded is flagged on_device but is no device pointer");
    if (expected_len && out_on_device && !hf_is_device_ptr(out)) return hf_fail(h, PGRC_E_PARAM, "decode: out is flagged on_device but is no device pointer");
    hipStream_t st = h->stream;
    int e;
    uint8_t props[4];
    if (coded_on_device) {
        HIP_TRY(h, hipMemcpyAsync(props, coded, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
    } else {
        memcpy(props, coded, 4);
    }
    if (props[0] == 1) return hf_fail(h, PGRC_E_PARAM, "decode: the frame is in FSE mode (mode byte 1), which this coder does not read");
    if (props[0] != 0) return hf_fail(h, PGRC_E_PARAM, "decode: unknown mode byte " + std::to_string(props[0]));
    const uint32_t order = props[1];
    if (order > PGRC_HUF_ORDER_MAX) return hf_fail(h, PGRC_E_PARAM, "decode: block order " + std::to_string(order) + " is above 17");
    if (!expected_len) {
        if (coded_len != 4) return hf_fail(h, PGRC_E_PARAM, "decode: bytes behind the props of an empty stream");
        return PGRC_OK;
    }
    const uint64_t nch = hf_chunks(expected_len, order);
    h->tm.chunks = (uint32_t)nch;
    if (nch > 0x7FFFFFFFull / 4 || coded_len < 4 + 4 * (nch - 1) + nch)
        return hf_fail(h, PGRC_E_PARAM, "decode: the frame of " + std::to_string(coded_len) + " bytes is too short for " + std::to_string(nch) + " chunks");
    const uint8_t *d_coded = (const uint8_t *)coded;
    if (!coded_on_device) {
        if ((e = pgrc_buf_unpooled(h, h->d_coded, coded_len))) return e;
        HIP_TRY(h, hipMemcpyAsync(h->d_coded.p, coded, coded_len, hipMemcpyHostToDevice, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        d_coded = (const uint8_t *)h->d_coded.p;
        h->tm.ms_upload = dec_ms_since(t0);
    }
    uint8_t *d_out = (uint8_t *)out;
    if (!out_on_device) {
        if ((e = pgrc_buf_unpooled(h, h->d_text, expected_len))) return e;
        d_out = (uint8_t *)h->d_text.p;
    }
    if ((e = pgrc_bufs_unpooled(h, {{&h->d_off, (nch + 1) * 8}, {&h->d_sizes, nch * 4}}))) return e;
    uint64_t *at = (uint64_t *)h->d_off.p;
    uint32_t *sizes = (uint32_t *)h->d_sizes.p, *flags = (uint32_t *)h->d_flag.p;      // flags[0 .. 2]: chunks by kind; flags[8]: the error word
    HIP_TRY(h, hipMemsetAsync(flags, 0, 64, st));
    HIP_TRY(h, h->ev.record(0, st));
    hipLaunchKernelGGL(k_huf_walk, dim3(1), dim3(1), 0, st, d_coded, coded_len, expected_len, order, nch, at, sizes, flags + 8);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, h->ev.record(1, st));
    uint32_t hf[16] = {};
    HIP_TRY(h, hipMemcpyAsync(hf, flags, 64, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (!hf[8]) {                                           // (the sizes are sound: every chunk lies inside the frame)
        hipLaunchKernelGGL(k_huf_decode, dim3((uint32_t)((nch + HF_TPB / 64 - 1) / (HF_TPB / 64))), dim3(HF_TPB), 0, st, d_coded, (const uint64_t *)at,
                           (const uint32_t *)sizes, expected_len, order, nch, d_out, flags + 8, flags);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, h->ev.record(2, st));
        HIP_TRY(h, hipMemcpyAsync(hf, flags, 64, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        h->tm.ms_emit = h->ev.ms(1, 2);
    }
    h->tm.ms_tables = h->ev.ms(0, 1);
    if (hf[8]) {
        const uint32_t code = hf[8] & 0xFFu;
        return hf_fail(h, PGRC_E_PARAM, "decode: chunk " + std::to_string(hf[8] >> 8) + ": " + (code < HF_E_COUNT ? HF_MESSAGES[code] : "damaged"));
    }
    h->tm.raw_chunks = hf[HF_RAW];
    h->tm.rle_chunks = hf[HF_RLE];
    h->tm.huf_chunks = hf[HF_HUF];
    if (!out_on_device) {
        const auto t1 = std::chrono::steady_clock::now();
        HIP_TRY(h, hipMemcpyAsync(out, d_out, expected_len, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        h->tm.ms_download = dec_ms_since(t1);
    }
    h->tm.ms_call = dec_ms_since(t0);
    return PGRC_OK;
}

} // extern "C"
