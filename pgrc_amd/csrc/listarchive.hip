// listarchive.hip -- the archive form of a reads list's mismatch streams on the device, both directions: the reshaping
// SeparatedPseudoGenomeOutputBuilder::compressedBuild does before its entropy coders (toStringAndSeparateZeros,
// SeparatedPseudoGenomePersistence.cpp:801-813; reorderingSymbolsExclusiveMismatchEncoding, :1115-1138;
// compressRlMisRevOffDest, :823-903) and the reassembly of ExtendedReadsListWithConstantAccessOption::
// loadConstantAccessExtendedReadsList (SeparatedExtendedReadsList.cpp:210-294).  include/pgrc_decode.h, "The archive form";
// DESIGN.md 4.17.  Restated, not translated: the reference's four serial loops fall apart into
//   zero flags, counts      scanops.h over "count != 0" (encode) / "flag == 0" (decode) and one scatter / gather
//   mismatch-list starts    the u64 sum scan of the counts that export.hip and decode.hip use
//   symbols                 k_la_hist: the low nibbles into five LDS bins per block (a sixth: a nibble above 4), one add of
//                           u64 per bin and block; the order is made on the host from the five numbers; k_la_recode: a
//                           25-entry table of 3-bit codes in two kernel arguments
//   the split               ONE stable radix-style pass on the digit mis_cnt, payloads of c bytes:
//     k_la_count     cnt[count][tile] over tiles of LA_TILE entries (bin-major, as radix.hip's k_rx_hist lays its matrix out);
//                    the zero counts are summed in registers: one LDS add per wave, not one per entry
//     scan           pgrc_ps_scan_u32 over the matrix; k_la_starts: the 256 totals, every count's first rank and, since every
//                    entry of destination c weighs c bytes, its start = the sum of c' * total[c'] over c' < c
//     k_la_scatter   ranks a tile's non-zero entries by count with the ballot peer groups of k_rx_scatter (per-wave LDS
//                    counters, waves in order) and copies entry e's c bytes from its mismatch-list start to
//                    start[c] + c * (matrix[c][tile] - first[c] + rank); k_la_gather: the same ranks, read instead of
//                    written, with convertMisRevOffsets2Offsets fused (k_dec_mis's loop)
// A group of 64 entries without a mismatch costs its count bytes and one ballot.  No global atomics in the split, no library
// kernel.  The 16-bit LDS counters hold at most LA_WSPAN = 1024 (a wave's entries) and LA_TILE = 8192 (a wave's offset).
// Positions in the destinations are 32-bit: n_mismatches < 2^32 and n_entries < 2^32 are required.
#include "ppchain.h"
#include "rlistctx.h"

#define LA_TPB 512
#define LA_NW (LA_TPB / 64)
#define LA_E 16
#define LA_TILE (LA_TPB * LA_E)
#define LA_WSPAN (64 * LA_E)
static_assert(LA_TILE == PGRC_LIST_ARCHIVE_TILE, "the header states the tile");
static_assert(LA_WSPAN <= 0xFFFF && LA_TILE <= 0xFFFF, "the LDS counters are 16 bits wide");

// the words of PgrcListArchive::small
#define LA_S_TOTAL 0            // u64[256]: entries per count
#define LA_S_START 256          // u64[256]: first byte of destination c among the destinations
#define LA_S_FIRST 512          // u64[256]: the scanned matrix value of (c, tile 0) = entries with a smaller count
#define LA_S_BINS 768           // u64[8]: the five value bins, bin 5 = codes with a nibble above 4
#define LA_S_WORDS 776

// ------------------------------------------------------------------------------------------------ kernels
struct LaNonZero { __device__ uint32_t operator()(uint8_t x) const { return x ? 1u : 0u; } };
struct LaIsZero { __device__ uint32_t operator()(uint8_t x) const { return x ? 0u : 1u; } };

// encode: zero_flags[i] = (cnt[i] == 0); the non-zero counts in entry order (inc: the inclusive scan of cnt != 0)
static __global__ void __launch_bounds__(PP_TPB) k_la_flags(const uint8_t *__restrict__ cnt, uint64_t n, const uint32_t *__restrict__ inc, uint8_t *__restrict__ zero_flags,
                                                            uint8_t *__restrict__ nonzero) {
    const uint64_t i = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (i >= n) return;
    const uint8_t c = cnt[i];
    zero_flags[i] = c ? 0 : 1;
    if (c) nonzero[inc[i] - 1u] = c;
}

// decode: cnt[i] = flag ? 0 : nonzero[its rank] (inc: the inclusive scan of flag == 0; its last value was checked against n_nonzero)
static __global__ void __launch_bounds__(PP_TPB) k_la_counts(const uint8_t *__restrict__ zero_flags, uint64_t n, const uint32_t *__restrict__ inc,
                                                             const uint8_t *__restrict__ nonzero, uint8_t *__restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (i >= n) return;
    cnt[i] = zero_flags[i] ? 0 : nonzero[inc[i] - 1u];
}

// the mismatch values of the context codes, five bins (+ one for a nibble above 4); 16 codes per lane and step
static __global__ void __launch_bounds__(PP_TPB) k_la_hist(const uint8_t *__restrict__ sym, uint64_t m, unsigned long long *__restrict__ bins) {
    __shared__ uint32_t s_bin[6];
    if (threadIdx.x < 6) s_bin[threadIdx.x] = 0;
    __syncthreads();
    uint32_t b[6] = {0, 0, 0, 0, 0, 0};
    auto one = [&](uint32_t c) {
        const uint32_t v = c & 15u, a = c >> 4;
        const uint32_t k = (v > 4u || a > 4u) ? 5u : v;
#pragma unroll
        for (uint32_t j = 0; j < 6; j++) b[j] += k == j;
    };
    const uint64_t lines = m >> 4;
    // (a block's lines per pass stay below 2^32 / 6 codes: the u32 bins of a block cannot wrap -- see the launch)
    for (uint64_t q = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x; q < lines; q += (uint64_t)gridDim.x * PP_TPB) {
        const uint4 v = ((const uint4 *)sym)[q];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int u = 0; u < 4; u++) one((w[j] >> (8 * u)) & 0xFFu);
    }
    if (blockIdx.x == 0 && threadIdx.x < (uint32_t)(m & 15)) one(sym[(lines << 4) + threadIdx.x]);
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) {
        uint32_t s = b[j];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&s_bin[j], s);
    }
    __syncthreads();
    if (threadIdx.x < 6 && s_bin[threadIdx.x]) atomicAdd(&bins[threadIdx.x], (unsigned long long)s_bin[threadIdx.x]);
}

// out[i] = table[actual * 5 + mismatch], the 25 entries 3 bits each: 0 .. 20 in lo, 21 .. 24 in hi (the nibbles were checked)
static __device__ __forceinline__ uint32_t la_code(uint32_t c, uint64_t lo, uint64_t hi) {
    const uint32_t a = min(c >> 4, 4u), v = min(c & 15u, 4u), j = a * 5u + v;
    return (uint32_t)((j < 21u ? lo >> (3u * j) : hi >> (3u * (j - 21u))) & 7u);
}
static __global__ void __launch_bounds__(PP_TPB) k_la_recode(const uint8_t *__restrict__ sym, uint64_t m, uint64_t lo, uint64_t hi, uint8_t *__restrict__ out) {
    const uint64_t q = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x, lines = m >> 4;
    if (q < lines) {
        const uint4 v = ((const uint4 *)sym)[q];
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t r = 0;
#pragma unroll
            for (int u = 0; u < 4; u++) r |= la_code((w[j] >> (8 * u)) & 0xFFu, lo, hi) << (8 * u);
            w[j] = r;
        }
        ((uint4 *)out)[q] = make_uint4(w[0], w[1], w[2], w[3]);
    } else if (q == lines) {
        for (uint64_t i = lines << 4; i < m; i++) out[i] = (uint8_t)la_code(sym[i], lo, hi);
    }
}

// decode: the exclusive codes are 0 .. 3 (k_dec_mis's check of form 0)
static __global__ void __launch_bounds__(PP_TPB) k_la_symcheck(const uint8_t *__restrict__ sym, uint64_t m, uint32_t *err) {
    uint32_t bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x; i < m; i += (uint64_t)gridDim.x * PP_TPB) bad |= sym[i] > 3u;
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(err, DEC_F_MISSYM);
}

// cnt[count][tile]: the tile's entries per count.  16 count bytes per lane; the zero counts are summed in registers, one LDS add per wave
static __global__ void __launch_bounds__(LA_TPB) k_la_count(const uint8_t *__restrict__ cnt, uint64_t n, uint64_t ntiles, uint32_t *__restrict__ mat) {
    __shared__ uint32_t hist[256];
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t tile = blockIdx.x, base = tile * LA_TILE + (uint64_t)threadIdx.x * LA_E;
    uint32_t zeros = 0;
    if (base + LA_E <= n) {
        const uint4 v = *(const uint4 *)(cnt + base);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t c = (w[j] >> (8 * u)) & 0xFFu;
                zeros += c == 0;
                if (c) atomicAdd(&hist[c], 1u);
            }
    } else {
        for (int k = 0; k < LA_E; k++) {
            const bool in = base + k < n;
            const uint32_t c = in ? cnt[base + k] : 1u;
            zeros += in && c == 0;
            if (in && c) atomicAdd(&hist[c], 1u);
        }
    }
    for (int o = 32; o > 0; o >>= 1) zeros += __shfl_down(zeros, o, 64);
    if ((threadIdx.x & 63) == 0 && zeros) atomicAdd(&hist[0], zeros);
    __syncthreads();
    if (threadIdx.x < 256) mat[(uint64_t)threadIdx.x * ntiles + tile] = hist[threadIdx.x];
}

// one block of 256 threads over the scanned matrix: small[TOTAL + c], small[FIRST + c], small[START + c]
static __global__ void __launch_bounds__(256) k_la_starts(const uint32_t *__restrict__ mat, uint64_t ntiles, uint64_t n, unsigned long long *__restrict__ small) {
    __shared__ uint64_t smem[4];
    const uint32_t c = threadIdx.x;
    const uint64_t first = mat[(uint64_t)c * ntiles], next = c < 255u ? (uint64_t)mat[(uint64_t)(c + 1u) * ntiles] : n;
    const uint64_t total = next - first;
    uint64_t all;
    const uint64_t start = sco_block_sum<4>((uint64_t)c * total, smem, &all);
    small[LA_S_TOTAL + c] = total;
    small[LA_S_FIRST + c] = first;
    small[LA_S_START + c] = start;
}

struct LaLds {
    uint16_t hist[LA_NW][256];      // per wave: running count (<= LA_WSPAN), then the wave's offset inside the tile's run (< LA_TILE)
    uint32_t pos[256];              // where the tile's run of count c starts among the destinations (bytes, < 2^32)
};

// Entries arrive as LA_E groups per wave; group i of wave w holds the tile's entries w * LA_WSPAN + i * 64 + lane, so "earlier
// wave, then earlier group, then lower lane" is the entry order -- the order in which equal counts leave.  rk[i]: count << 16
// | rank inside the wave.
static __device__ __forceinline__ void la_rank_tile(LaLds &s, const uint8_t *__restrict__ cnt, uint64_t t0, uint32_t nvalid, uint32_t (&rk)[LA_E]) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int i = 0; i < LA_E; i++) {
        const uint32_t x = wv * LA_WSPAN + (uint32_t)i * 64u + lane;
        const uint32_t c = x < nvalid ? cnt[t0 + x] : 0u;
        const bool valid = c != 0;
        unsigned long long peers = __ballot(valid);
        uint32_t rank = 0;
        if (peers) {                                    // (uniform: a group without a mismatch ends here)
#pragma unroll
            for (uint32_t b = 0; b < 8; b++) {
                const unsigned long long bal = __ballot((c >> b) & 1u);
                peers &= ((c >> b) & 1u) ? bal : ~bal;
            }
            // the lowest lane of every peer group advances the wave's counter of that count
            const uint32_t leader = valid ? (uint32_t)__ffsll((long long)peers) - 1u : lane;
            uint32_t old = 0;
            if (valid && lane == leader) {
                old = s.hist[wv][c];
                s.hist[wv][c] = (uint16_t)(old + (uint32_t)__popcll(peers));
            }
            old = __shfl(old, leader, 64);
            rank = old + (uint32_t)__popcll(peers & lt);
        }
        rk[i] = c << 16 | rank;
    }
}

// the waves' counts -> their offsets inside the count's run; the run's first byte among the destinations
static __device__ __forceinline__ void la_tile_starts(LaLds &s, const uint32_t *__restrict__ mat, uint64_t ntiles, uint64_t tile,
                                                      const unsigned long long *__restrict__ small) {
    if (threadIdx.x < 256) {
        const uint32_t c = threadIdx.x;
        uint32_t tot = 0;
        for (uint32_t w = 0; w < LA_NW; w++) {
            const uint32_t t = s.hist[w][c];
            s.hist[w][c] = (uint16_t)tot;
            tot += t;
        }
        const uint64_t before = (uint64_t)mat[(uint64_t)c * ntiles + tile] - small[LA_S_FIRST + c];
        s.pos[c] = (uint32_t)(small[LA_S_START + c] + (uint64_t)c * before);
    }
}

static __device__ __forceinline__ void la_clear(LaLds &s) {
    for (uint32_t x = threadIdx.x; x < LA_NW * 256; x += LA_TPB) (&s.hist[0][0])[x] = (uint16_t)0;
}

// encode: entry e's c offsets, in stream order, to destination c
static __global__ void __launch_bounds__(LA_TPB) k_la_scatter(const uint8_t *__restrict__ cnt, uint64_t n, uint64_t ntiles, const uint32_t *__restrict__ mat,
                                                              const unsigned long long *__restrict__ small, const uint64_t *__restrict__ mcum,
                                                              const uint8_t *__restrict__ off_in, uint8_t *__restrict__ dest) {
    __shared__ LaLds s;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t tile = blockIdx.x, t0 = tile * LA_TILE;
    const uint32_t nvalid = (uint32_t)min((uint64_t)LA_TILE, n - t0);
    la_clear(s);
    __syncthreads();
    uint32_t rk[LA_E];
    la_rank_tile(s, cnt, t0, nvalid, rk);
    __syncthreads();
    la_tile_starts(s, mat, ntiles, tile, small);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < LA_E; i++) {
        const uint32_t c = rk[i] >> 16;
        if (!c) continue;
        const uint64_t e = t0 + wv * LA_WSPAN + (uint32_t)i * 64u + lane;
        const uint8_t *src = off_in + mcum[e];
        uint8_t *dst = dest + (s.pos[c] + c * ((uint32_t)s.hist[wv][c] + (rk[i] & 0xFFFFu)));
        for (uint32_t k = 0; k < c; k++) dst[k] = src[k];
    }
}

// decode: entry e's c offsets from source c (SPLIT) or from the one stream at its mismatch-list start, as forward offsets
// (convertMisRevOffsets2Offsets: walking the stream, pos -= r + 1 yields the entry's offsets from the last to the first)
template <bool SPLIT>
static __global__ void __launch_bounds__(LA_TPB) k_la_gather(const uint8_t *__restrict__ cnt, uint64_t n, uint64_t ntiles, const uint32_t *__restrict__ mat,
                                                             const unsigned long long *__restrict__ small, const uint64_t *__restrict__ mcum,
                                                             const uint8_t *__restrict__ src_all, uint32_t L, uint8_t *__restrict__ moff, uint32_t *err) {
    __shared__ LaLds s;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t tile = blockIdx.x, t0 = tile * LA_TILE;
    const uint32_t nvalid = (uint32_t)min((uint64_t)LA_TILE, n - t0);
    uint32_t rk[LA_E];
    if (SPLIT) {
        la_clear(s);
        __syncthreads();
        la_rank_tile(s, cnt, t0, nvalid, rk);
        __syncthreads();
        la_tile_starts(s, mat, ntiles, tile, small);
        __syncthreads();
    } else {
#pragma unroll
        for (int i = 0; i < LA_E; i++) {
            const uint32_t x = wv * LA_WSPAN + (uint32_t)i * 64u + lane;
            rk[i] = (x < nvalid ? (uint32_t)cnt[t0 + x] : 0u) << 16;
        }
    }
    uint32_t bad = 0;
#pragma unroll
    for (int i = 0; i < LA_E; i++) {
        const uint32_t c = rk[i] >> 16;
        if (!c) continue;
        const uint64_t e = t0 + wv * LA_WSPAN + (uint32_t)i * 64u + lane;
        const uint64_t ms = mcum[e];
        const uint8_t *src = SPLIT ? src_all + (s.pos[c] + c * ((uint32_t)s.hist[wv][c] + (rk[i] & 0xFFFFu))) : src_all + ms;
        int32_t p = (int32_t)L;
        for (uint32_t k = 0; k < c; k++) {
            p -= (int32_t)src[k] + 1;
            int32_t o = p;
            if (o < 0) { bad = DEC_F_MISOFF; o = 0; }
            moff[ms + c - 1u - k] = (uint8_t)o;
        }
    }
    if (bad) atomicOr(err, bad);
}

// ------------------------------------------------------------------------------------------------ host side
static int la_fail(PgrcStage *d, const char *who, const std::string &msg) { return dec_fail(d, PGRC_E_PARAM, std::string("list archive (") + who + "): " + msg); }

// count matrix of the n counts at `cnt`, scanned; the per-count words in `small` and (synchronised) at h_small
static int la_matrix(PgrcStage *d, PgrcListArchive &st, const uint8_t *cnt, uint64_t n, uint64_t *ntiles_out, uint64_t (&h_small)[LA_S_BINS]) {
    const uint64_t ntiles = std::max<uint64_t>(1, (n + LA_TILE - 1) / LA_TILE), cells = ntiles * 256;
    int e;
    if ((e = pgrc_bufs_unpooled(d, {{&st.mat, cells * 4 + 16}, {&st.fold, pgrc_ps_scan_blocks(cells) * 4 + 16}}))) return e;
    uint32_t *mat = (uint32_t *)st.mat.p;
    hipLaunchKernelGGL(k_la_count, dim3((uint32_t)ntiles), dim3(LA_TPB), 0, d->stream, cnt, n, ntiles, mat);
    HIP_TRY(d, hipGetLastError());
    if ((e = pgrc_ps_scan_u32(d, d->stream, mat, cells, (uint32_t *)st.fold.p))) return e;
    hipLaunchKernelGGL(k_la_starts, dim3(1), dim3(256), 0, d->stream, (const uint32_t *)mat, ntiles, n, (unsigned long long *)st.small.p);
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, hipMemcpyAsync(h_small, st.small.p, sizeof(h_small), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    *ntiles_out = ntiles;
    return PGRC_OK;
}

// reorderingSymbolsExclusiveMismatchEncoding's order: std::sort of five elements is an insertion sort (stable) by descending count
static void la_symbol_order(const uint64_t counts[5], uint8_t order[5], uint8_t rev[5]) {
    for (int i = 0; i < 5; i++) order[i] = (uint8_t)i;
    for (int i = 1; i < 5; i++) {
        const uint8_t v = order[i];
        int j = i;
        while (j > 0 && counts[v] > counts[order[j - 1]]) {
            order[j] = order[j - 1];
            j--;
        }
        order[j] = v;
    }
    for (int i = 0; i < 5; i++) rev[order[i]] = (uint8_t)i;
}

// where the streams start in the block (device and host alike): flags | codes | destinations | non-zero counts | props
struct LaLayout {
    uint64_t at_flags, at_sym, at_dest, at_nz;
};
static LaLayout la_layout(uint64_t n, uint64_t m) {
    LaLayout o;
    o.at_flags = 0;
    o.at_sym = dec_a16(n) + 16;
    o.at_dest = o.at_sym + dec_a16(m) + 16;
    o.at_nz = o.at_dest + dec_a16(m) + 16;
    return o;
}

// what the device part of the encoder hands to the host part
struct LaEncoded {
    uint32_t n_nonzero = 0, limit = 0;
    uint8_t order[5] = {};
    uint64_t h_small[LA_S_BINS] = {};
};

// the device side of the encoder: cnt (n), sym and off (m each) lie in device memory, complete on d->stream; the block is
// written at ob (la_layout; room for at_nz + n + 16 bytes).  The caller has recorded ev[0].
static int la_encode_device(PgrcStage *d, PgrcListArchive &st, const uint8_t *cnt, const uint8_t *sym, const uint8_t *off, uint64_t n, uint64_t m, bool fast, uint8_t *ob, LaEncoded *res) {
    static const char *who = "encode";
    int e;
    const LaLayout lay = la_layout(n, m);
    if ((e = pgrc_bufs_unpooled(d, {{&st.inc, n * 4 + 16}, {&st.mcum, (n + 1) * 8}, {&st.small, LA_S_WORDS * 8}}))) return e;
    uint32_t *inc = (uint32_t *)st.inc.p;
    uint64_t *mcum = (uint64_t *)st.mcum.p;
    unsigned long long *small = (unsigned long long *)st.small.p;
    HIP_TRY(d, hipMemsetAsync(small, 0, LA_S_WORDS * 8, d->stream));

    // flags, non-zero counts, mismatch-list starts
    uint32_t n_nonzero = 0;
    uint64_t m_dev = 0;
    if (n) {
        if ((e = pgrc_buf_unpooled(d, d->scratch, sco_scratch_elems(n) * sizeof(uint64_t)))) return e;
        HIP_TRY(d, sco_scan<true>(d->stream, (const uint8_t *)cnt, inc, n, LaNonZero{}, ScoPlus{}, 0u, (uint32_t *)d->scratch.p));
        hipLaunchKernelGGL(k_la_flags, dim3(pp_grid(n)), dim3(PP_TPB), 0, d->stream, (const uint8_t *)cnt, n, (const uint32_t *)inc, ob + lay.at_flags, ob + lay.at_nz);
        HIP_TRY(d, hipGetLastError());
        HIP_TRY(d, hipMemcpyAsync(&n_nonzero, inc + n - 1, 4, hipMemcpyDeviceToHost, d->stream));
    }
    if ((e = dec_scan<false>(d, XfU8{cnt}, n, 0, mcum))) return e;
    HIP_TRY(d, hipMemcpyAsync(&m_dev, mcum + n, 8, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, st.ev.record(1, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    // nothing below reads a code or an offset before the counts are known to describe the streams
    if (m_dev != m) return la_fail(d, who, "n_mismatches is " + std::to_string(m) + ", the counts sum to " + std::to_string(m_dev));

    // symbols
    HIP_TRY(d, st.ev.record(2, d->stream));
    uint64_t h_bins[8] = {};
    if (m) {
        // 2048 blocks at most, and each bin of a block below 2^32: a block sees m / blocks + 4096 codes at most
        const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((m >> 4) + PP_TPB - 1) / PP_TPB, 2048));
        hipLaunchKernelGGL(k_la_hist, dim3(grid), dim3(PP_TPB), 0, d->stream, (const uint8_t *)sym, m, small + LA_S_BINS);
        HIP_TRY(d, hipGetLastError());
        HIP_TRY(d, hipMemcpyAsync(h_bins, small + LA_S_BINS, sizeof(h_bins), hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(d, hipStreamSynchronize(d->stream));
        if (h_bins[5]) return la_fail(d, who, std::to_string(h_bins[5]) + " mismatch codes with a nibble above 4");
    }
    uint8_t order[5], rev[5];
    la_symbol_order(h_bins, order, rev);
    if (m) {
        uint64_t lo = 0, hi = 0;
        for (uint32_t a = 0; a < 5; a++)
            for (uint32_t v = 0; v < 5; v++) {
                const uint32_t j = a * 5 + v;
                const uint64_t code = (uint64_t)(rev[v] - (rev[v] > rev[a] ? 1 : 0));
                if (j < 21) lo |= code << (3 * j);
                else hi |= code << (3 * (j - 21));
            }
        hipLaunchKernelGGL(k_la_recode, dim3(pp_grid((m >> 4) + 1)), dim3(PP_TPB), 0, d->stream, (const uint8_t *)sym, m, lo, hi, ob + lay.at_sym);
        HIP_TRY(d, hipGetLastError());
    }
    HIP_TRY(d, st.ev.record(3, d->stream));

    // the split
    uint64_t h_small[LA_S_BINS] = {};
    uint32_t limit = 0;
    if (fast) {
        limit = 1;
        if (m) HIP_TRY(d, hipMemcpyAsync(ob + lay.at_dest, off, m, hipMemcpyDeviceToDevice, d->stream));
    } else if (n) {
        uint64_t ntiles = 0;
        if ((e = la_matrix(d, st, cnt, n, &ntiles, h_small))) return e;
        if (h_small[LA_S_TOTAL + 255]) return la_fail(d, who, std::to_string(h_small[LA_S_TOTAL + 255]) + " entries with 255 mismatches (the reference's map has 255 elements)");
        for (uint32_t c = 1; c < 255; c++)
            if (h_small[LA_S_TOTAL + c]) limit = c;
        if (m) hipLaunchKernelGGL(k_la_scatter, dim3((uint32_t)ntiles), dim3(LA_TPB), 0, d->stream, (const uint8_t *)cnt, n, ntiles, (const uint32_t *)st.mat.p,
                                  (const unsigned long long *)small, (const uint64_t *)mcum, (const uint8_t *)off, ob + lay.at_dest);
        HIP_TRY(d, hipGetLastError());
    }
    HIP_TRY(d, st.ev.record(4, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));

    res->n_nonzero = n_nonzero;
    res->limit = limit;
    memcpy(res->order, order, 5);
    memcpy(res->h_small, h_small, sizeof(h_small));
    return PGRC_OK;
}

// the streams of a block that lies at blk in host memory; the props, which the host makes, go behind the non-zero counts
static void la_describe(pgrc_list_archive_streams *out, uint8_t *blk, uint64_t n, uint64_t m, bool fast, const LaEncoded &r) {
    const LaLayout lay = la_layout(n, m);
    const uint32_t limit = r.limit;
    out->struct_size = sizeof(pgrc_list_archive_streams);
    out->n_entries = n;
    out->n_mismatches = m;
    out->n_nonzero = r.n_nonzero;
    out->zero_flags = blk;
    out->nonzero_cnt = blk + lay.at_nz;
    out->mis_sym = blk + lay.at_sym;
    for (int i = 0; i < 5; i++) out->bases_order[i] = "ACGTN"[r.order[i]];
    uint8_t *props = blk + lay.at_nz + dec_a16(r.n_nonzero) + 16;
    props[0] = (uint8_t)limit;
    for (uint32_t c = 1; c < limit; c++) props[c] = (uint8_t)c;
    out->props = props;
    out->props_len = std::max(1u, limit);
    out->n_dests = limit;
    if (fast) {
        out->dest[1] = blk + lay.at_dest;
        out->dest_len[1] = m;
    } else {
        for (uint32_t c = 1; c <= limit; c++) {
            out->dest[c] = blk + lay.at_dest + r.h_small[LA_S_START + c];
            out->dest_len[c] = (uint64_t)c * r.h_small[LA_S_TOTAL + c];
        }
    }
}

uint64_t pgrc_la_device_bytes(uint64_t n, uint64_t m) { return la_layout(n, m).at_nz + n + 16; }
uint64_t pgrc_la_host_bytes(uint64_t n, uint64_t m) { return la_layout(n, m).at_nz + dec_a16(n) + 16 + 256; }

int pgrc_la_encode_resident(PgrcStage *d, PgrcListArchive &st, const uint8_t *d_cnt, const uint8_t *d_sym, const uint8_t *d_off, uint64_t n, uint64_t m, bool fast, uint8_t *d_block,
                            PgrcLaResident *res) {
    int e;
    if ((e = st.ev.ensure(d))) return e;
    HIP_TRY(d, st.ev.record(0, d->stream));
    LaEncoded r;
    if ((e = la_encode_device(d, st, d_cnt, d_sym, d_off, n, m, fast, d_block, &r))) return e;
    res->down = la_layout(n, m).at_nz + r.n_nonzero;
    res->n_nonzero = r.n_nonzero;
    res->limit = r.limit;
    memcpy(res->order, r.order, 5);
    memcpy(res->h_small, r.h_small, sizeof(r.h_small));
    static_assert(sizeof(res->h_small) == sizeof(r.h_small), "rlistctx.h states the words");
    return PGRC_OK;
}

void pgrc_la_describe_resident(pgrc_list_archive_streams *out, uint8_t *blk, uint64_t n, uint64_t m, bool fast, const PgrcLaResident *res) {
    LaEncoded r;
    r.n_nonzero = res->n_nonzero;
    r.limit = res->limit;
    memcpy(r.order, res->order, 5);
    memcpy(r.h_small, res->h_small, sizeof(r.h_small));
    la_describe(out, blk, n, m, fast, r);
}

static int la_encode_run(PgrcStage *d, PgrcListArchive &st, const pgrc_export_streams *in, bool fast, pgrc_list_archive_streams *out) {
    const uint64_t n = in->n_entries, m = in->n_mismatches;
    const auto t0 = std::chrono::steady_clock::now();
    int e;
    if ((e = st.ev.ensure(d))) return e;
    const LaLayout lay = la_layout(n, m);
    const uint64_t sym_at = dec_a16(n) + 16, off_at = sym_at + dec_a16(m) + 16;
    if ((e = pgrc_bufs_unpooled(d, {{&st.in, off_at + m + 16}, {&st.out, lay.at_nz + n + 16}}))) return e;
    uint8_t *ib = (uint8_t *)st.in.p, *ob = (uint8_t *)st.out.p;
    uint8_t *cnt = ib, *sym = ib + sym_at, *off = ib + off_at;
    if ((e = dec_upload_host(d, cnt, in->mis_cnt, n)) || (e = dec_upload_host(d, sym, in->mis_sym, m)) || (e = dec_upload_host(d, off, in->mis_rev_off, m))) return e;
    HIP_TRY(d, st.ev.record(0, d->stream));
    const float ms_upload = dec_ms_since(t0);
    LaEncoded r;
    if ((e = la_encode_device(d, st, cnt, sym, off, n, m, fast, ob, &r))) return e;
    const uint32_t n_nonzero = r.n_nonzero, limit = r.limit;

    // one page-locked block, one copy: everything the device made; the props are the host's
    const auto t1 = std::chrono::steady_clock::now();
    const uint64_t at_props = lay.at_nz + dec_a16(n_nonzero) + 16;
    const DecBlockLayout<1> h = {{0}, {lay.at_nz + n_nonzero}, at_props + 256};
    const void *src[1] = {ob};
    uint8_t *blk = nullptr;
    uint64_t down = 0;
    if ((e = dec_download_block(d, "list archive (encode)", h, src, &blk, &down))) return e;
    la_describe(out, blk, n, m, fast, r);
    out->block = blk;
    pgrc_list_archive_timing &t = st.tm;
    t = pgrc_list_archive_timing{};
    t.struct_size = sizeof(pgrc_list_archive_timing);
    t.encode = 1;
    t.ms_upload = ms_upload;
    t.ms_flags_device = st.ev.ms(0, 1);
    t.ms_symbols_device = st.ev.ms(2, 3);
    t.ms_split_device = st.ev.ms(3, 4);
    t.ms_download = dec_ms_since(t1);
    t.ms_call = dec_ms_since(t0);
    t.bytes_up = n + 2 * m;
    t.bytes_down = down;
    t.n_nonzero = n_nonzero;
    t.limit = limit;
    st.have_timing = true;
    return PGRC_OK;
}

// the mismatch tables of a list from the archive's streams (the middle of pgrc_dec_add_list)
int pgrc_la_tables(pgrc_decode_ctx *d, pgrc_decode_ctx::List &l, const pgrc_list_archive_streams *s) {
    static const char *who = "add_list_archive";
    const uint64_t n = s->n_entries, m = s->n_mismatches, nz = s->n_nonzero;
    const auto t0 = std::chrono::steady_clock::now();
    PgrcListArchive &st = d->la;
    st.have_timing = false;
    // the checks that need no device
    if (n != l.n) return la_fail(d, who, "n_entries differs from the list's");
    if (n >= (1ull << 32) || m >= (1ull << 32)) return la_fail(d, who, "2^32 entries or mismatches or more");
    if (nz > n) return la_fail(d, who, "more non-zero counts than entries");
    if ((n && !s->zero_flags) || (nz && !s->nonzero_cnt) || (m && !s->mis_sym)) return la_fail(d, who, "a NULL stream with a non-zero count");
    if (!s->props || s->props_len < 1) return la_fail(d, who, "no props");
    const uint32_t limit = s->props[0];
    if (limit > 254) return la_fail(d, who, "props: a limit above 254");
    if (s->props_len != std::max(1u, limit) || s->n_dests != limit) return la_fail(d, who, "props: props_len / n_dests do not belong to the limit");
    for (uint32_t c = 1; c < limit; c++)
        if (s->props[c] != c) return la_fail(d, who, "props: a map other than the identity (the reference writes no other)");
    uint64_t sum = 0;
    for (uint32_t c = 1; c <= limit; c++) {
        if (s->dest_len[c] > m) return la_fail(d, who, "a destination longer than n_mismatches");
        if (s->dest_len[c] && !s->dest[c]) return la_fail(d, who, "a NULL destination with a non-zero length");
        sum += s->dest_len[c];
    }
    if (sum != m) return la_fail(d, who, "the destinations hold " + std::to_string(sum) + " bytes, n_mismatches is " + std::to_string(m));
    int e;
    if ((e = st.ev.ensure(d))) return e;
    // uploads: flags | non-zero counts in `in`, the codes straight into the list, the sources one behind the other in `out`
    const uint64_t nz_at = dec_a16(n) + 16;
    if ((e = pgrc_bufs_unpooled(d, {{&st.in, nz_at + nz + 16}, {&st.inc, n * 4 + 16}, {&st.cnt, n + 16}, {&st.small, LA_S_WORDS * 8}, {&st.out, m + 16},
                                    {&l.mcum, (n + 1) * 8}, {&l.moff, m}, {&l.msym, m}})))
        return e;
    uint8_t *flags = (uint8_t *)st.in.p, *nonzero = flags + nz_at, *cnt = (uint8_t *)st.cnt.p, *src = (uint8_t *)st.out.p;
    uint32_t *inc = (uint32_t *)st.inc.p;
    uint64_t *mcum = (uint64_t *)l.mcum.p;
    unsigned long long *small = (unsigned long long *)st.small.p;
    if ((e = dec_upload_host(d, flags, s->zero_flags, n)) || (e = dec_upload_host(d, nonzero, s->nonzero_cnt, nz)) || (e = dec_upload_host(d, l.msym.p, s->mis_sym, m))) return e;
    uint64_t h_start[256] = {};
    uint64_t at = 0;
    for (uint32_t c = 1; c <= limit; c++) {
        h_start[c] = at;
        if ((e = dec_upload_host(d, src + at, s->dest[c], s->dest_len[c]))) return e;
        at += s->dest_len[c];
    }
    HIP_TRY(d, st.ev.record(0, d->stream));
    const float ms_upload = dec_ms_since(t0);

    // counts from the flags; mismatch-list starts
    uint32_t n_clear = 0;
    uint64_t m_dev = 0;
    if (n) {
        if ((e = pgrc_buf_unpooled(d, d->scratch, sco_scratch_elems(n) * sizeof(uint64_t)))) return e;
        HIP_TRY(d, sco_scan<true>(d->stream, (const uint8_t *)flags, inc, n, LaIsZero{}, ScoPlus{}, 0u, (uint32_t *)d->scratch.p));
        HIP_TRY(d, hipMemcpyAsync(&n_clear, inc + n - 1, 4, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(d, hipStreamSynchronize(d->stream));
    }
    // no non-zero count is read before their number is known to be the flags'
    if (n_clear != nz) return la_fail(d, who, std::to_string(n_clear) + " entries without a zero flag, n_nonzero is " + std::to_string(nz));
    if (n) hipLaunchKernelGGL(k_la_counts, dim3(pp_grid(n)), dim3(PP_TPB), 0, d->stream, (const uint8_t *)flags, n, (const uint32_t *)inc, (const uint8_t *)nonzero, cnt);
    HIP_TRY(d, hipGetLastError());
    if ((e = dec_scan<false>(d, XfU8{cnt}, n, 0, mcum))) return e;
    HIP_TRY(d, hipMemcpyAsync(&m_dev, mcum + n, 8, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, st.ev.record(1, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    if (m_dev != m) return la_fail(d, who, "n_mismatches is " + std::to_string(m) + ", the counts sum to " + std::to_string(m_dev));
    l.nmis = m;

    // the codes
    HIP_TRY(d, st.ev.record(2, d->stream));
    if (m) hipLaunchKernelGGL(k_la_symcheck, dim3((uint32_t)std::min<uint64_t>(pp_grid(m), 4096)), dim3(PP_TPB), 0, d->stream, (const uint8_t *)l.msym.p, m, (uint32_t *)d->flag.p);
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, st.ev.record(3, d->stream));

    // the gather.  limit <= 1: every count reads the one source at its mismatch-list start (its length is m: checked above)
    if (m) {
        const uint64_t ntiles1 = (n + LA_TILE - 1) / LA_TILE;
        if (limit <= 1) {
            if (limit == 0) return la_fail(d, who, "a count above the limit 0");   // (m != 0 with no destination cannot pass the sum check; kept for the reader)
            hipLaunchKernelGGL(k_la_gather<false>, dim3((uint32_t)ntiles1), dim3(LA_TPB), 0, d->stream, (const uint8_t *)cnt, n, ntiles1, (const uint32_t *)nullptr,
                               (const unsigned long long *)nullptr, (const uint64_t *)mcum, (const uint8_t *)src, d->L, (uint8_t *)l.moff.p, (uint32_t *)d->flag.p);
        } else {
            uint64_t h_small[LA_S_BINS] = {}, ntiles = 0;
            if ((e = la_matrix(d, st, cnt, n, &ntiles, h_small))) return e;
            // nothing is gathered before every source is known to hold exactly its entries
            for (uint32_t c = limit + 1; c < 256; c++)
                if (h_small[LA_S_TOTAL + c]) return la_fail(d, who, "a count of " + std::to_string(c) + ", above the limit " + std::to_string(limit));
            for (uint32_t c = 1; c <= limit; c++) {
                if (s->dest_len[c] != (uint64_t)c * h_small[LA_S_TOTAL + c])
                    return la_fail(d, who, "source " + std::to_string(c) + " holds " + std::to_string(s->dest_len[c]) + " bytes for " + std::to_string(h_small[LA_S_TOTAL + c]) + " entries");
                if (h_small[LA_S_START + c] != h_start[c]) return dec_fail(d, PGRC_E_DEVICE, "list archive (add_list_archive): the sources' starts disagree");
            }
            hipLaunchKernelGGL(k_la_gather<true>, dim3((uint32_t)ntiles), dim3(LA_TPB), 0, d->stream, (const uint8_t *)cnt, n, ntiles, (const uint32_t *)st.mat.p,
                               (const unsigned long long *)small, (const uint64_t *)mcum, (const uint8_t *)src, d->L, (uint8_t *)l.moff.p, (uint32_t *)d->flag.p);
        }
        HIP_TRY(d, hipGetLastError());
    }
    HIP_TRY(d, st.ev.record(4, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    pgrc_list_archive_timing &t = st.tm;
    t = pgrc_list_archive_timing{};
    t.struct_size = sizeof(pgrc_list_archive_timing);
    t.encode = 0;
    t.ms_upload = ms_upload;
    t.ms_flags_device = st.ev.ms(0, 1);
    t.ms_symbols_device = st.ev.ms(2, 3);
    t.ms_split_device = st.ev.ms(3, 4);
    t.bytes_up = n + nz + 2 * m;
    t.n_nonzero = nz;
    t.limit = limit;
    return PGRC_OK;
}

extern "C" {

int pgrc_list_archive_encode(pgrc_decode_ctx *d, const pgrc_export_streams *in, int32_t fast_level, pgrc_list_archive_streams *out) {
    static const char *who = "encode";
    if (!d) return PGRC_E_PARAM;
    if (!out) return la_fail(d, who, "out is NULL");
    *out = pgrc_list_archive_streams{};
    if (!in) return la_fail(d, who, "in is NULL");
    if (in->off_width != 1) return la_fail(d, who, "offsets of " + std::to_string(in->off_width) + " bytes (the archive's loader reads one byte each)");
    if (in->n_entries >= (1ull << 32) || in->n_mismatches >= (1ull << 32)) return la_fail(d, who, "2^32 entries or mismatches or more");
    if ((in->n_entries && !in->mis_cnt) || (in->n_mismatches && (!in->mis_sym || !in->mis_rev_off))) return la_fail(d, who, "a NULL stream with a non-zero count");
    PGRC_ON_DEVICE(d);
    d->la.have_timing = false;
    const int e = la_encode_run(d, d->la, in, fast_level != 0, out);
    if (e) *out = pgrc_list_archive_streams{};
    return e;
}

void pgrc_list_archive_free(pgrc_list_archive_streams *s) {
    if (!s) return;
    if (s->block) (void)hipHostFree(s->block);
    *s = pgrc_list_archive_streams{};
}

int pgrc_decode_add_list_archive(pgrc_decode_ctx *d, const pgrc_decode_list *list, const pgrc_list_archive_streams *s) {
    if (!d) return PGRC_E_PARAM;
    if (!s || s->struct_size != sizeof(pgrc_list_archive_streams)) return la_fail(d, "add_list_archive", "streams is NULL or struct_size is not sizeof(pgrc_list_archive_streams)");
    const auto t0 = std::chrono::steady_clock::now();
    d->la.have_timing = false;
    const int e = pgrc_dec_add_list(d, list, s);
    if (e) return e;
    d->la.tm.ms_call = dec_ms_since(t0);
    d->la.have_timing = true;
    return PGRC_OK;
}

int pgrc_list_archive_get_timing(pgrc_decode_ctx *d, pgrc_list_archive_timing *out) {
    if (!d) return PGRC_E_PARAM;
    if (!out || out->struct_size != sizeof(pgrc_list_archive_timing)) return dec_fail(d, PGRC_E_PARAM, "timing is NULL or struct_size is not sizeof(pgrc_list_archive_timing)");
    if (!d->la.have_timing) return dec_fail(d, PGRC_E_STATE, "no list-archive call has succeeded on this context");
    *out = d->la.tm;
    return PGRC_OK;
}

}   // extern "C"
