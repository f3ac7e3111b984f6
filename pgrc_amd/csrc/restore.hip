// restore.hip -- the restore of the matched pseudogenomes on the device (pgrc_decode_set_mapped_text,
// include/pgrc_decode.h): the inverse of the Pg-vs-Pg marking (row f2), as decode.hip is the inverse of the export.
//
// Reference behaviour restated (not translated):
//   SimplePgMatcher::restoreMatchedPgs / restoreMatchedPg     matching/SimplePgMatcher.cpp:259-351
//   SimplePgMatcher::markAndRemoveExactMatches (the encoder)  matching/SimplePgMatcher.cpp:65-144
//   readUIntByteFrugal                                        utils/helper.h:209-219
//   reverseComplement, complementsLut                         utils/helper.cpp:247-276, :395-403
//
// The reference appends mark by mark into one growing string.  Here, per part (HQ, LQ, N):
//   parse     the '%' positions of the mapped text and the ends of the byte-frugal values (bytes < 128) are counted per
//             block with 16-byte loads, the block counts are scanned, and a second pass writes every mark's mapped
//             position and assembles every value from its at most 10 bytes; the offsets are read at fixed width.  A
//             scan of the match lengths gives every mark's output position: mapped position - mark rank + the lengths
//             of the earlier matches.  Every check of the header runs here, before anything is installed.
//   literals  every aligned 8-byte word of the output is made by one lane: from two aligned 8-byte loads of the mapped
//             text, funnel-shifted, when the word lies inside one literal run; byte by byte at the edges of runs
//   matches   HQ marks copy from earlier HQ output, so a matched symbol's source may itself be matched (chains, with
//             a reverse complement at every hop).  Every matched symbol gets a pointer to its source -- another matched
//             symbol, or a terminal literal byte of the mapped text -- and pointer jumping (Wyllie) halves the chains'
//             depth per pass until every pointer is terminal: ceil(log2(depth)) passes.  Hop class: a matched symbol
//             is at least one hop from its origin x, so the class is its hop parity -- odd gives c(x), even gives
//             c(c(x)), which is NOT x for lower case, U and bytes outside complementsLut.  LQ and N then copy from the
//             finished HQ in one hop.
#include <chrono>

#include "decctx.h"
#include "varlenctx.h"

#define RS_WPB 1024                      // 16-byte words per block of the parse passes (4 per lane)
#define RS_SPT 16                        // matched symbols per lane of the symbol kernels
#define RS_LPT 4                         // output 8-byte words per lane of the literal kernel
#define RS_PAD 16                        // zero bytes after every part and stream on the device
#define RS_TERM (1ull << 63)             // pointer: terminal (index = mapped-text position) ...
#define RS_PAR (1ull << 62)              // ... parity of the hops to it
#define RS_IDX (RS_PAR - 1)

// error flags of the device checks
#define RS_F_LONG 1u                     // a byte-frugal value of more than 10 bytes
#define RS_F_END 2u                      // a byte-frugal value runs past its stream's end
#define RS_F_SRC 4u                      // a source range reaches past the HQ end
#define RS_F_SELF 8u                     // an HQ source reaches its own output position

struct XfU64 { const uint64_t *p; __device__ uint64_t operator()(uint64_t i) const { return p[i]; } };

// per-byte flags (bit 7 of each byte) of a 32-bit word: MODE 0 byte == '%', MODE 1 byte < 128 (a byte-frugal value's end)
template <int MODE>
__device__ __forceinline__ uint32_t rs_hits(uint32_t w) {
    if (MODE == 1) return ~w & 0x80808080u;
    const uint32_t x = w ^ 0x25252525u;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}

// the hits of 16-byte word q of buf (n bytes), as a 16-bit mask (bit b = byte 16q + b)
template <int MODE>
__device__ __forceinline__ uint32_t rs_word_mask(const uint8_t *__restrict__ buf, uint64_t n, uint64_t q) {
    if (16 * q >= n) return 0;
    const uint4 v = ((const uint4 *)buf)[q];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t h = rs_hits<MODE>(w[k]);
        m |= (((h >> 7) & 1u) | ((h >> 14) & 2u) | ((h >> 21) & 4u) | ((h >> 28) & 8u)) << (4 * k);
    }
    const uint64_t left = n - 16 * q;
    if (left < 16) m &= (1u << left) - 1u;
    return m;
}

template <int MODE>
__global__ void __launch_bounds__(DEC_TPB) k_rs_count(const uint8_t *__restrict__ buf, uint64_t n, uint64_t *__restrict__ bsum) {
    __shared__ uint64_t smem[DEC_TPB / 64];
    uint64_t s = 0;
    for (uint32_t v = 0; v < RS_WPB / DEC_TPB; v++)
        s += __popc(rs_word_mask<MODE>(buf, n, (uint64_t)blockIdx.x * RS_WPB + v * DEC_TPB + threadIdx.x));
    uint64_t tot;
    sco_block_sum<DEC_TPB / 64>(s, smem, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// MODE 0: out[rank] = position of the mark.  MODE 1: out[rank] = the value ending at that byte (its bytes run back over
// the bytes >= 128 before it; the earliest is the lowest 7-bit group).
template <int MODE>
__global__ void __launch_bounds__(DEC_TPB) k_rs_write(const uint8_t *__restrict__ buf, uint64_t n, const uint64_t *__restrict__ bex,
                                                      uint64_t *__restrict__ out, uint32_t *err) {
    __shared__ uint64_t smem[DEC_TPB / 64];
    uint64_t base = bex[blockIdx.x];
    uint32_t bad = 0;
    for (uint32_t v = 0; v < RS_WPB / DEC_TPB; v++) {
        const uint64_t q = (uint64_t)blockIdx.x * RS_WPB + v * DEC_TPB + threadIdx.x;
        uint32_t m = rs_word_mask<MODE>(buf, n, q);
        uint64_t tot;
        uint64_t r = base + sco_block_sum<DEC_TPB / 64>((uint64_t)__popc(m), smem, &tot);
        base += tot;
        while (m) {
            const uint32_t b = __ffs(m) - 1;
            m &= m - 1;
            const uint64_t i = 16 * q + b;
            if (MODE == 0) {
                out[r++] = i;
            } else {
                uint64_t val = buf[i];
                uint32_t k = 1;
                for (; k <= i && k < 10; k++) {
                    const uint32_t c = buf[i - k];
                    if (c < 128) break;
                    val = (val << 7) | (c & 127u);
                }
                if (k <= i && k == 10 && buf[i - k] >= 128) bad |= RS_F_LONG;
                out[r++] = val;
            }
        }
        if (MODE == 1 && n && q == (n - 1) / 16 && buf[n - 1] >= 128) bad |= RS_F_END;
    }
    if (bad) atomicOr(err, bad);
}

struct RsPart {                          // device view of one part (kernel argument)
    const uint8_t *mapped;               // the part's mapped text (16-byte aligned, zero padded)
    const uint8_t *offs;                 // its offsets stream
    const uint64_t *vals;                // its byte-frugal values: minMatchLength, then one per mark
    uint64_t *mpos, *len, *off, *cum, *opos;   // per mark: mapped position, match length, source offset, exclusive
                                               // scan of the lengths (n+1), output position in the part
    uint64_t n;                          // marks
    uint64_t lim;                        // LQ / N: the HQ length (sources end at or before it)
    uint64_t tbase, tlen;                // the part's place in the joined text
    uint32_t width, hq;
};

__global__ void k_rs_marks(RsPart p) {
    const uint32_t minlen = (uint32_t)p.vals[0];          // (the reference reads minMatchLength into a uint32_t)
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < p.n; k += (uint64_t)gridDim.x * blockDim.x) {
        p.len[k] = p.vals[k + 1] + minlen;
        uint64_t o = 0;
        for (uint32_t b = 0; b < p.width; b++) o |= (uint64_t)p.offs[k * p.width + b] << (8 * b);
        p.off[k] = o;
    }
}

__global__ void k_rs_check(RsPart p, uint32_t *err) {
    uint32_t bad = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < p.n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t o = p.mpos[k] - k + p.cum[k];
        p.opos[k] = o;
        const uint64_t lim = p.hq ? o : p.lim;
        if (p.off[k] > lim || p.len[k] > lim - p.off[k]) bad |= p.hq ? RS_F_SELF : RS_F_SRC;
    }
    if (bad) atomicOr(err, bad);
}

// the first index i of a[0, n) with a[i] > key (n when none)
__device__ __forceinline__ uint64_t rs_upper(const uint64_t *__restrict__ a, uint64_t n, uint64_t key) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] <= key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one lane: RS_LPT aligned 8-byte words of the joined text, the part's bytes among them; literal bytes only (the match
// bytes are left to the match kernels)
__global__ void __launch_bounds__(DEC_TPB) k_rs_literals(RsPart p, uint8_t *__restrict__ text) {
    const uint64_t w0 = (p.tbase >> 3) + ((uint64_t)blockIdx.x * DEC_TPB + threadIdx.x) * RS_LPT;
    const uint64_t end = p.tbase + p.tlen;
    if (8 * w0 >= end) return;
    const uint64_t *src64 = (const uint64_t *)((uintptr_t)p.mapped & ~(uintptr_t)7);
    const uint32_t mis = (uint32_t)((uintptr_t)p.mapped & 7);  // (0: the parts are 16-byte aligned; kept general)
    uint64_t q = (8 * w0 > p.tbase ? 8 * w0 : p.tbase) - p.tbase;   // part-local position of the lane's first byte
    uint64_t r = rs_upper(p.opos, p.n, q);                        // marks at or before q
    for (uint32_t u = 0; u < RS_LPT; u++) {
        const uint64_t a0 = 8 * (w0 + u);
        if (a0 >= end) break;
        // the fast path: all 8 bytes in the part and in literal run r
        if (a0 >= p.tbase && a0 + 8 <= end) {
            q = a0 - p.tbase;
            while (r < p.n && p.opos[r] <= q) r++;
            const bool after_prev = r == 0 || q >= p.opos[r - 1] + p.len[r - 1];
            const bool before_next = r == p.n || q + 8 <= p.opos[r];
            if (after_prev && before_next) {
                const uint64_t i = q - p.cum[r] + r + mis, sh = 8 * (i & 7);
                const uint64_t lo = src64[i >> 3];
                const uint64_t v = sh ? (lo >> sh) | (src64[(i >> 3) + 1] << (64 - sh)) : lo;
                *(uint64_t *)(text + a0) = v;
                continue;
            }
        }
        for (uint32_t b = 0; b < 8; b++) {
            const uint64_t a = a0 + b;
            if (a < p.tbase || a >= end) continue;
            q = a - p.tbase;
            while (r < p.n && p.opos[r] <= q) r++;
            if (r > 0 && q < p.opos[r - 1] + p.len[r - 1]) continue;
            text[a] = p.mapped[q - p.cum[r] + r];
        }
    }
}

// The source position of matched symbol j of mark k
__device__ __forceinline__ uint64_t rs_src(const RsPart &p, uint64_t k, uint64_t j, int rc) {
    return rc ? p.off[k] + p.len[k] - 1 - j : p.off[k] + j;
}

// HQ: the pointer of every matched symbol g (g = cum[k] + j): to the matched symbol its source is, or, terminal, to the
// literal byte of the mapped text it is; parity 1 (one hop).  flag: set when a pointer is not terminal.
__global__ void __launch_bounds__(DEC_TPB) k_rs_ptr_init(RsPart p, int rc, uint64_t *__restrict__ ptr, uint32_t *more) {
    const uint64_t total = p.cum[p.n];
    const uint64_t g0 = ((uint64_t)blockIdx.x * DEC_TPB + threadIdx.x) * RS_SPT;
    uint32_t nonterm = 0;
    if (g0 < total) {
        uint64_t k = rs_upper(p.cum, p.n, g0) - 1;     // the last mark with cum[k] <= g0 (cum[0] = 0 <= g0)
        uint64_t r = ~0ull;
        const uint64_t gend = min(total, g0 + RS_SPT);
        for (uint64_t g = g0; g < gend; g++) {
            bool fresh = r == ~0ull;
            while (g >= p.cum[k + 1]) { k++; fresh = true; }
            const uint64_t sp = rs_src(p, k, g - p.cum[k], rc);
            if (fresh) r = rs_upper(p.opos, p.n, sp);
            while (r > 0 && p.opos[r - 1] > sp) r--;
            while (r < p.n && p.opos[r] <= sp) r++;
            uint64_t v;
            if (r > 0 && sp < p.opos[r - 1] + p.len[r - 1]) {
                v = (p.cum[r - 1] + sp - p.opos[r - 1]) | RS_PAR;
                nonterm = 1;
            } else {
                v = (sp - p.cum[r] + r) | RS_PAR | RS_TERM;
            }
            ptr[g] = v;
        }
    }
    if (__any(nonterm) && (threadIdx.x & 63) == 0) atomicOr(more, 1u);
}

// one pointer-jumping pass: every non-terminal pointer jumps to its target's pointer, the parities add up
__global__ void __launch_bounds__(DEC_TPB) k_rs_jump(uint64_t *ptr, uint64_t total, uint32_t *more) {
    uint32_t nonterm = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * DEC_TPB + threadIdx.x; g < total; g += (uint64_t)gridDim.x * DEC_TPB) {
        const uint64_t v = __hip_atomic_load(ptr + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v & RS_TERM) continue;
        const uint64_t u = __hip_atomic_load(ptr + (v & RS_IDX), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t nv = (u & ~RS_PAR) | ((u ^ v) & RS_PAR);
        __hip_atomic_store(ptr + g, nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        nonterm |= !(nv & RS_TERM);
    }
    if (__any(nonterm) && (threadIdx.x & 63) == 0) atomicOr(more, 1u);
}

// the matched symbols of a part.  HQ (ptr != NULL): from the terminal pointers, c(x) for odd, c(c(x)) for even hops.
// LQ / N: one hop from the finished HQ at the start of the joined text.
__global__ void __launch_bounds__(DEC_TPB) k_rs_fill(RsPart p, int rc, const uint64_t *__restrict__ ptr, uint8_t *__restrict__ text) {
    __shared__ uint8_t s_comp[256];
    s_comp[threadIdx.x] = dec_complement(threadIdx.x);
    __syncthreads();
    const uint64_t total = p.cum[p.n];
    const uint64_t g0 = ((uint64_t)blockIdx.x * DEC_TPB + threadIdx.x) * RS_SPT;
    if (g0 >= total) return;
    uint64_t k = rs_upper(p.cum, p.n, g0) - 1;
    const uint64_t gend = min(total, g0 + RS_SPT);
    for (uint64_t g = g0; g < gend; g++) {
        while (g >= p.cum[k + 1]) k++;
        const uint64_t j = g - p.cum[k];
        uint32_t c;
        if (ptr) {
            const uint64_t v = ptr[g];
            c = p.mapped[v & RS_IDX];
            if (rc) c = (v & RS_PAR) ? s_comp[c] : s_comp[s_comp[c]];
        } else {
            c = text[rs_src(p, k, j, rc)];
            if (rc) c = s_comp[c];
        }
        text[p.tbase + p.opos[k] + j] = (uint8_t)c;
    }
}

// ------------------------------------------------------------------------------------------------ host side
static uint64_t rs_a16(uint64_t x) { return (x + 15) & ~15ull; }

static int rs_fail(pgrc_decode_ctx *d, const std::string &msg) { return dec_fail(d, PGRC_E_PARAM, "set_mapped_text: " + msg); }

static uint32_t rs_grid(uint64_t items, uint64_t per_block) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + per_block - 1) / per_block, 1u << 30));
}

// pgrc_decode_set_mapped_text (v == NULL: the mapped text comes as bytes in m->mapped) and pgrc_decode_set_mapped_text_coded
// (the coded bytes go up and varlen.hip decodes them in HBM; the parts then reach their places by device copies)
static int rs_set_mapped(pgrc_decode_ctx *d, const pgrc_decode_mapped *m, pgrc_varlen *v, const void *coded, uint64_t coded_len) {
    if (!m || m->struct_size != sizeof(pgrc_decode_mapped))
        return dec_fail(d, PGRC_E_PARAM, "mapped is NULL or struct_size is not sizeof(pgrc_decode_mapped)");
    d->have_text = false;
    d->have_parts = false;
    d->nl = 0;
    d->have_order = false;
    d->tm = pgrc_decode_timing{};
    const uint64_t mtot = m->mapped_len[0] + m->mapped_len[1] + m->mapped_len[2];
    if (v) {
        if (m->mapped) return rs_fail(d, "mapped must be NULL when the text comes coded");
        if (coded_len && !coded) return rs_fail(d, "coded is NULL");
        if (v->device != d->device) return rs_fail(d, "the coder is on another device");
    } else if (mtot && !m->mapped) return rs_fail(d, "mapped is NULL");
    for (int p = 0; p < 3; p++)
        if ((m->map_off_bytes[p] && !m->map_off[p]) || (m->map_len_bytes[p] && !m->map_len[p])) return rs_fail(d, "a stream is NULL");
    PGRC_ON_DEVICE(d);
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t width = m->org_hq_len <= UINT32_MAX ? 4 : 8;
    const int rc = m->rev_compl ? 1 : 0;
    int e;

    // 1. upload: every part and stream at a 16-byte aligned place, RS_PAD zero bytes after each
    // byte arrays: 0..2 the parts, 3..5 the offsets streams, 6..8 the lengths streams
    const uint8_t *hsrc[9];
    uint64_t nbytes[9], at[9], dev_bytes = 0;
    uint64_t mo = 0, part_at[3];
    for (int p = 0; p < 3; p++) {
        part_at[p] = mo;
        hsrc[p] = v ? nullptr : (const uint8_t *)m->mapped + mo;
        nbytes[p] = m->mapped_len[p];
        mo += m->mapped_len[p];
        hsrc[3 + p] = m->map_off[p];
        nbytes[3 + p] = m->map_off_bytes[p];
        hsrc[6 + p] = m->map_len[p];
        nbytes[6 + p] = m->map_len_bytes[p];
    }
    for (int s = 0; s < 9; s++) {
        at[s] = dev_bytes;
        dev_bytes += rs_a16(nbytes[s] + RS_PAD);
    }
    if ((e = pgrc_buf_unpooled(d, d->rs_mapped, dev_bytes))) return e;
    uint8_t *dm = (uint8_t *)d->rs_mapped.p;
    if (v) {
        if ((e = pgrc_buf_unpooled(d, d->rs_coded, coded_len)) || (e = pgrc_buf_unpooled(d, d->rs_join, mtot))) return e;
        if ((e = dec_upload_host(d, d->rs_coded.p, coded, coded_len))) return e;
        HIP_TRY(d, hipStreamSynchronize(d->stream));
        if ((e = pgrc_varlen_decode(v, d->rs_coded.p, coded_len, 1, mtot, d->rs_join.p, 1)))
            return dec_fail(d, e, std::string("set_mapped_text_coded: ") + pgrc_varlen_last_error(v));
    }
    for (int s = 0; s < 9; s++) {
        const uint64_t z = nbytes[s] & ~15ull;
        HIP_TRY(d, hipMemsetAsync(dm + at[s] + z, 0, rs_a16(nbytes[s] + RS_PAD) - z, d->stream));
        if (!nbytes[s]) continue;
        if (s < 3 && v) HIP_TRY(d, hipMemcpyAsync(dm + at[s], (const uint8_t *)d->rs_join.p + part_at[s], nbytes[s], hipMemcpyDeviceToDevice, d->stream));
        else if ((e = s < 3 ? dec_upload_host(d, dm + at[s], hsrc[s], nbytes[s]) : dec_upload(d, dm + at[s], hsrc[s], nbytes[s]))) return e;   // (the streams: always staged)
    }
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    pgrc_decode_restore_timing tm{};
    tm.struct_size = sizeof(tm);
    tm.ms_upload = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();

    // 2. parse: count the marks (parts) and the value ends (lengths streams) per block, scan the block counts
    if ((e = dec_clear_err(d))) return e;
    HIP_TRY(d, hipEventRecord(d->ev_a, d->stream));
    const int job_buf[6] = {0, 1, 2, 6, 7, 8};
    uint64_t nb[6], bs_at[6], bs_words = 0;
    for (int j = 0; j < 6; j++) {
        nb[j] = (nbytes[job_buf[j]] + 16 * RS_WPB - 1) / (16 * RS_WPB);
        bs_at[j] = bs_words;
        bs_words += 2 * nb[j] + 1;                       // block counts, then their exclusive scan (nb + 1)
    }
    if ((e = pgrc_buf_unpooled(d, d->rs_bsum, bs_words * 8))) return e;
    uint64_t *bs = (uint64_t *)d->rs_bsum.p;
    for (int j = 0; j < 6; j++) {
        const int s = job_buf[j];
        if (nb[j]) {
            if (j < 3) hipLaunchKernelGGL(k_rs_count<0>, dim3((uint32_t)nb[j]), dim3(DEC_TPB), 0, d->stream, dm + at[s], nbytes[s], bs + bs_at[j]);
            else hipLaunchKernelGGL(k_rs_count<1>, dim3((uint32_t)nb[j]), dim3(DEC_TPB), 0, d->stream, dm + at[s], nbytes[s], bs + bs_at[j]);
        }
        if ((e = dec_scan<false>(d, XfU64{bs + bs_at[j]}, nb[j], 0, bs + bs_at[j] + nb[j]))) return e;
    }
    HIP_TRY(d, hipGetLastError());
    uint64_t cnt[6];
    for (int j = 0; j < 6; j++) HIP_TRY(d, hipMemcpyAsync(&cnt[j], bs + bs_at[j] + 2 * nb[j], 8, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    static const char *pname[3] = {"HQ", "LQ", "N"};
    for (int p = 0; p < 3; p++) {
        const uint64_t n = cnt[p], nv = cnt[3 + p];
        if (nv ? nv != n + 1 : n != 0)
            return rs_fail(d, std::string(pname[p]) + ": " + std::to_string(n) + " marks but " + std::to_string(nv) +
                                  " byte-frugal values (minMatchLength and one per mark)");
        if (nbytes[3 + p] != n * width)
            return rs_fail(d, std::string(pname[p]) + ": the offsets stream holds " + std::to_string(nbytes[3 + p]) + " bytes, not " +
                                  std::to_string(n) + " x " + std::to_string(width));
    }
    // per-mark arrays: mpos, len, off, cum (n+1), opos; the values (n+1)
    uint64_t mk_at[3], val_at[3], mk_words = 0, val_words = 0;
    for (int p = 0; p < 3; p++) {
        mk_at[p] = mk_words;
        mk_words += 5 * cnt[p] + 1;
        val_at[p] = val_words;
        val_words += cnt[p] + 1;
    }
    if ((e = pgrc_buf_unpooled(d, d->rs_marks, mk_words * 8)) || (e = pgrc_buf_unpooled(d, d->rs_vals, val_words * 8))) return e;
    RsPart part[3];
    uint32_t *flag = (uint32_t *)d->flag.p;
    for (int p = 0; p < 3; p++) {
        const uint64_t n = cnt[p];
        RsPart &x = part[p];
        x = RsPart{};
        x.mapped = dm + at[p];
        x.offs = dm + at[3 + p];
        uint64_t *v = (uint64_t *)d->rs_vals.p + val_at[p];
        x.vals = v;
        uint64_t *mk = (uint64_t *)d->rs_marks.p + mk_at[p];
        x.mpos = mk;
        x.len = mk + n;
        x.off = mk + 2 * n;
        x.cum = mk + 3 * n;
        x.opos = mk + 4 * n + 1;
        x.n = n;
        x.lim = m->org_hq_len;
        x.width = width;
        x.hq = p == 0;
        if (!cnt[3 + p]) HIP_TRY(d, hipMemsetAsync(v, 0, 8, d->stream));      // an empty lengths stream: minMatchLength 0
        if (nb[p])
            hipLaunchKernelGGL(k_rs_write<0>, dim3((uint32_t)nb[p]), dim3(DEC_TPB), 0, d->stream, dm + at[p], nbytes[p],
                               (const uint64_t *)(bs + bs_at[p] + nb[p]), x.mpos, flag);
        if (nb[3 + p])
            hipLaunchKernelGGL(k_rs_write<1>, dim3((uint32_t)nb[3 + p]), dim3(DEC_TPB), 0, d->stream, dm + at[6 + p], nbytes[6 + p],
                               (const uint64_t *)(bs + bs_at[3 + p] + nb[3 + p]), v, flag);
        if (n) hipLaunchKernelGGL(k_rs_marks, dim3(rs_grid(n, 256)), dim3(256), 0, d->stream, x);
        if ((e = dec_scan<false>(d, XfU64{x.len}, n, 0, x.cum))) return e;
        if (n) hipLaunchKernelGGL(k_rs_check, dim3(rs_grid(n, 256)), dim3(256), 0, d->stream, x, flag);
    }
    HIP_TRY(d, hipGetLastError());
    uint64_t matched[3];
    uint32_t f = 0;
    for (int p = 0; p < 3; p++) HIP_TRY(d, hipMemcpyAsync(&matched[p], part[p].cum + cnt[p], 8, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipMemcpyAsync(&f, flag, 4, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipEventRecord(d->ev_b, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    tm.ms_parse_device = dec_elapsed(d->ev_a, d->ev_b);
    if (f) {
        std::string msg;
        if (f & RS_F_LONG) msg += " a byte-frugal value is longer than 10 bytes;";
        if (f & RS_F_END) msg += " a byte-frugal value runs past its stream's end;";
        if (f & RS_F_SRC) msg += " an LQ / N source range reaches past the HQ end;";
        if (f & RS_F_SELF) msg += " an HQ source range reaches its own output position;";
        return rs_fail(d, msg);
    }
    uint64_t plen[3], total = 0;
    for (int p = 0; p < 3; p++) {
        plen[p] = nbytes[p] - cnt[p] + matched[p];
        part[p].tbase = total;
        part[p].tlen = plen[p];
        total += plen[p];
    }
    if (plen[0] != m->org_hq_len)
        return rs_fail(d, "the restored HQ holds " + std::to_string(plen[0]) + " symbols, not org_hq_len = " + std::to_string(m->org_hq_len));

    // 3. literals into the text buffer (padded as pgrc_decode_set_text pads it)
    const uint64_t tbytes = rs_a16(total) + DEC_TEXT_PAD;
    if ((e = pgrc_buf_unpooled(d, d->text, tbytes))) return e;
    uint8_t *text = (uint8_t *)d->text.p;
    HIP_TRY(d, hipMemsetAsync(text + (total & ~15ull), 0, tbytes - (total & ~15ull), d->stream));
    HIP_TRY(d, hipEventRecord(d->ev_a, d->stream));
    for (int p = 0; p < 3; p++)
        if (plen[p]) {
            const uint64_t words = ((part[p].tbase + plen[p] + 7) >> 3) - (part[p].tbase >> 3);
            hipLaunchKernelGGL(k_rs_literals, dim3(rs_grid(words, (uint64_t)DEC_TPB * RS_LPT)), dim3(DEC_TPB), 0, d->stream, part[p], text);
        }
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, hipEventRecord(d->ev_b, d->stream));

    // 4. matches: HQ chains by pointer jumping, then the HQ fill, then LQ and N in one hop from the finished HQ
    uint32_t passes = 0;
    if (matched[0]) {
        if ((e = pgrc_buf_unpooled(d, d->rs_ptr, matched[0] * 8))) return e;
        uint64_t *ptr = (uint64_t *)d->rs_ptr.p;
        if ((e = dec_clear_err(d))) return e;
        hipLaunchKernelGGL(k_rs_ptr_init, dim3(rs_grid(matched[0], (uint64_t)DEC_TPB * RS_SPT)), dim3(DEC_TPB), 0, d->stream, part[0], rc, ptr, flag);
        HIP_TRY(d, hipGetLastError());
        const uint32_t jgrid = rs_grid(matched[0], (uint64_t)DEC_TPB * 16);
        for (;;) {
            uint32_t more = 0;
            HIP_TRY(d, hipMemcpyAsync(&more, flag, 4, hipMemcpyDeviceToHost, d->stream));
            HIP_TRY(d, hipStreamSynchronize(d->stream));
            if (!more) break;
            if (passes > 64) return dec_fail(d, PGRC_E_DEVICE, "set_mapped_text: HQ chains did not resolve in 64 passes");
            if ((e = dec_clear_err(d))) return e;
            hipLaunchKernelGGL(k_rs_jump, dim3(jgrid), dim3(DEC_TPB), 0, d->stream, ptr, matched[0], flag);
            HIP_TRY(d, hipGetLastError());
            passes++;
        }
        hipLaunchKernelGGL(k_rs_fill, dim3(rs_grid(matched[0], (uint64_t)DEC_TPB * RS_SPT)), dim3(DEC_TPB), 0, d->stream, part[0], rc,
                           (const uint64_t *)ptr, text);
    }
    for (int p = 1; p < 3; p++)
        if (matched[p])
            hipLaunchKernelGGL(k_rs_fill, dim3(rs_grid(matched[p], (uint64_t)DEC_TPB * RS_SPT)), dim3(DEC_TPB), 0, d->stream, part[p], rc,
                               (const uint64_t *)nullptr, text);
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, hipEventRecord(d->ev_k0[0], d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    tm.ms_literals_device = dec_elapsed(d->ev_a, d->ev_b);
    tm.ms_matches_device = dec_elapsed(d->ev_b, d->ev_k0[0]);
    tm.passes = passes;
    for (int p = 0; p < 3; p++) {
        tm.marks[p] = cnt[p];
        tm.matched[p] = matched[p];
        d->part_len[p] = plen[p];
    }
    d->text_len = total;
    d->have_text = true;
    d->have_parts = true;
    tm.ms_call = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    d->rtm = tm;
    return PGRC_OK;
}

extern "C" {

int pgrc_decode_set_mapped_text(pgrc_decode_ctx *d, const pgrc_decode_mapped *m) {
    if (!d) return PGRC_E_PARAM;
    return rs_set_mapped(d, m, nullptr, nullptr, 0);
}

int pgrc_decode_set_mapped_text_coded(pgrc_decode_ctx *d, const pgrc_decode_mapped *m, pgrc_varlen *v, const void *coded, uint64_t coded_len) {
    if (!d) return PGRC_E_PARAM;
    if (!v) return dec_fail(d, PGRC_E_PARAM, "set_mapped_text_coded: the coder is NULL");
    return rs_set_mapped(d, m, v, coded, coded_len);
}

int pgrc_decode_text_lengths(pgrc_decode_ctx *d, uint64_t lens[3]) {
    if (!d || !lens) return PGRC_E_PARAM;
    if (!d->have_parts) return dec_fail(d, PGRC_E_STATE, "text_lengths: the text did not come from set_mapped_text");
    for (int p = 0; p < 3; p++) lens[p] = d->part_len[p];
    return PGRC_OK;
}

int pgrc_decode_get_text(pgrc_decode_ctx *d, uint64_t first, uint64_t n, char *out) {
    if (!d) return PGRC_E_PARAM;
    if (!d->have_text) return dec_fail(d, PGRC_E_STATE, "get_text before a text is set");
    if (first > d->text_len || n > d->text_len - first) return dec_fail(d, PGRC_E_PARAM, "get_text: bytes beyond the text end");
    if (!n) return PGRC_OK;
    if (!out) return dec_fail(d, PGRC_E_PARAM, "out is NULL");
    PGRC_ON_DEVICE(d);
    const uint8_t *src = (const uint8_t *)d->text.p + first;
    if (pgrc_host_pinned(out)) {
        HIP_TRY(d, hipMemcpyAsync(out, src, n, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(d, hipStreamSynchronize(d->stream));
        return PGRC_OK;
    }
    // pieces through the two staging buffers: piece c is copied down while piece c-1 is handed over
    int pend = -1;
    uint64_t pend_off = 0, pend_bytes = 0;
    for (uint64_t o = 0, c = 0; o < n; o += DEC_STAGE_BYTES, c++) {
        const int k = (int)(c & 1);
        const uint64_t b = std::min<uint64_t>(DEC_STAGE_BYTES, n - o);
        HIP_TRY(d, hipMemcpyAsync(d->stage[k], src + o, b, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(d, hipEventRecord(d->ev_copied[k], d->stream));
        if (pend >= 0) {
            HIP_TRY(d, hipEventSynchronize(d->ev_copied[pend]));
            memcpy(out + pend_off, d->stage[pend], pend_bytes);
        }
        pend = k;
        pend_off = o;
        pend_bytes = b;
    }
    HIP_TRY(d, hipEventSynchronize(d->ev_copied[pend]));
    memcpy(out + pend_off, d->stage[pend], pend_bytes);
    return PGRC_OK;
}

int pgrc_decode_get_restore_timing(pgrc_decode_ctx *d, pgrc_decode_restore_timing *out) {
    if (!d || !out) return PGRC_E_PARAM;
    if (out->struct_size != sizeof(pgrc_decode_restore_timing))
        return dec_fail(d, PGRC_E_PARAM, "struct_size is not sizeof(pgrc_decode_restore_timing)");
    *out = d->rtm;
    out->struct_size = sizeof(pgrc_decode_restore_timing);
    return PGRC_OK;
}

}   // extern "C"
