// pgasm.hip -- the assembly of a pseudogenome from the overlap graph on the device: what the reference's generator does after
// findOverlappingReads (AbstractOverlapPseudoGenomeGenerator.cpp: removeCyclesAndPrepareComponents :6-41,
// countPseudoGenomeLength :146-153, assemblePseudoGenomeTemplate :183-219) and applyIndexesMapping
// (include/pgrc_assemble.h).
//
// The reference chases one pointer per read through three arrays and copies a suffix per read.  Here it falls apart into
//   pred, checks       one scatter pred[next[i]] = i with the range checks; one pass that finds every i in pred[next[i]] (a read
//                      with two predecessors loses a slot) and compares the suffix of row i with the prefix of row next[i]
//   cycles             pointer jumping on next, in place, on 64-bit words (pointer, largest index passed): a path runs out within
//                      ceil(log2(R + 1)) + 1 passes, what is live then lies on a cycle and knows its largest index; the read that
//                      is that index cuts its link
//   ranking            the same jumping on pred with (head, distance)
//   lists              a tail writes its chain's length at the head, scanops.h turns the lengths into the chains' first
//                      entries, every read lands at base[head] + distance: walk order, shift, off and orgIdx in one scatter;
//                      the 64-bit scan of the shifts is where every entry's symbols start
//   text               a block owns a tile of the text, finds its entries by binary search in the starts, unpacks the first
//                      `shift` symbols of each from its packed row into LDS and stores the tile in 16-byte lanes
// Integer work bound by random 4- and 8-byte accesses per read and one random row gather; no library kernel, no atomic with
// a returned value.
#include <chrono>

#include "asmctx.h"
#include "decctx.h"
#include "devutil.h"
#include "pgrc_assemble.h"
#include "rlistctx.h"

#define AS_TPB 256
#define AS_TILE 8192u           // text bytes of a block: two 16-byte lanes per thread
#define AS_CHUNK 8u             // row bytes of one work item of the text kernel (32 symbols of ACGT, 24 of ACGNT)

// the words of `bad`, in the order the refusals are reported
enum { AS_BAD_NEXT, AS_BAD_PRED, AS_BAD_OVL, AS_BAD_OVL_END, AS_BAD_LINK, AS_BAD_ROW, AS_BAD_WORDS };
// the words of `cnt` (u64)
enum { AS_CNT_CYCLES, AS_CNT_LOST, AS_CNT_COMPONENTS, AS_CNT_SINGLES, AS_CNT_WORDS };

struct pgrc_asm_ctx {
    // The stage handle, and a decode context because the assembled text is one's text: pgrc_decode_get_text reads it, and it
    // ends in the padding the row kernels expect (text, text_len, have_text; the read length is that of the last run)
    pgrc_decode_ctx *d = nullptr;
    DevBuf rows, nx, ovraw, ov, pred, st, len, walk, sh, off, org, start, map, fold, words, packed;
    PhaseEvents<7> ev;
    uint32_t symbols = 0;
    bool have_packed = false, have_timing = false;
    // the reads list of the last successful run where it lies (org, off): its entries, and whether the run applied a host mapping
    uint64_t list_n = 0;
    bool list_mapped = false;
    pgrc_asm_timing tm{};
};

static DevBufList as_bufs(pgrc_asm_ctx *a) {
    return {&a->rows, &a->nx, &a->ovraw, &a->ov, &a->pred, &a->st, &a->len, &a->walk, &a->sh, &a->off, &a->org, &a->start, &a->map, &a->fold, &a->words, &a->packed};
}

// ------------------------------------------------------------------------------------------------ kernels
// symbol x of a packed row: its code in the alphabet's order ("ACGT" / "ACGNT"), first symbol most significant
__device__ __forceinline__ uint32_t as_code(const uint8_t *__restrict__ row, uint32_t x, bool five) {
    if (!five) return ((uint32_t)row[x >> 2] >> (6u - 2u * (x & 3u))) & 3u;
    const uint32_t v = row[x / 3u], k = x % 3u;
    return k == 0 ? v / 25u : k == 1 ? (v / 5u) % 5u : v % 5u;
}
__device__ __forceinline__ uint8_t as_ascii(uint32_t code, bool five) {
    return (uint8_t)(five ? (0x544E474341ull >> (8u * code)) & 0xFFu : code2ascii(code));
}

// pred[next[i]] = i; the overlaps widened to 16 bits.  bad: next > R, overlap > L, an overlap without a successor
static __global__ void __launch_bounds__(AS_TPB) k_as_pred(const uint32_t *__restrict__ nx, const void *__restrict__ ovraw, uint32_t width, uint64_t R, uint32_t L,
                                                           uint32_t *__restrict__ pred, uint16_t *__restrict__ ov, uint32_t *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * AS_TPB + threadIdx.x;
    if (i > R) return;
    if (i == 0) {
        ov[0] = 0;
        return;
    }
    const uint32_t n = nx[i], o = width == 1 ? ((const uint8_t *)ovraw)[i] : ((const uint16_t *)ovraw)[i];
    if (n > R) bad[AS_BAD_NEXT] = 1;
    else if (n) pred[n] = (uint32_t)i;
    if (o > L) bad[AS_BAD_OVL] = 1;
    if (o && !n) bad[AS_BAD_OVL_END] = 1;
    ov[i] = (uint16_t)o;
}

// every link: i is the predecessor pred knows of next[i], and the last overlap[i] symbols of row i are the first of row next[i]
static __global__ void __launch_bounds__(AS_TPB) k_as_link(const uint8_t *__restrict__ rows, uint32_t rb, uint32_t symbols, uint32_t L, const uint32_t *__restrict__ nx,
                                                           const uint16_t *__restrict__ ov, const uint32_t *__restrict__ pred, uint64_t R, uint32_t *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * AS_TPB + threadIdx.x;
    if (i == 0 || i > R) return;
    const uint32_t n = nx[i], o = ov[i];
    if (!n || n > R) return;
    if (pred[n] != (uint32_t)i) bad[AS_BAD_PRED] = 1;
    if (o > L) return;
    const uint8_t *a = rows + (i - 1) * rb, *b = rows + (uint64_t)(n - 1) * rb;
    const bool five = symbols == 5;
    const uint32_t from = L - o;
    bool differ = false;
    for (uint32_t k = 0; k < o; k++) differ |= as_code(a, from + k, five) != as_code(b, k, five);
    if (differ) bad[AS_BAD_LINK] = 1;
}

// ACGNT rows: a byte of 125 or more is no three digits, and the digits after symbol L - 1 are zero
static __global__ void __launch_bounds__(AS_TPB) k_as_rows5(const uint8_t *__restrict__ rows, uint64_t total, uint32_t rb, uint32_t L, uint32_t *__restrict__ bad) {
    const uint32_t tail = L % 3u;
    for (uint64_t g = (uint64_t)blockIdx.x * AS_TPB + threadIdx.x; g < total; g += (uint64_t)gridDim.x * AS_TPB) {
        const uint32_t v = rows[g];
        bool no = v >= 125u;
        if (tail && g % rb == rb - 1u) no |= (tail == 1 ? v % 25u : v % 5u) != 0;
        if (no) bad[AS_BAD_ROW] = 1;
    }
}

// st[i] = (next[i], i): the pointer, and the largest index from i up to (not including) the pointer's read
static __global__ void __launch_bounds__(AS_TPB) k_as_cyc_init(const uint32_t *__restrict__ nx, uint64_t R, uint64_t *__restrict__ st) {
    const uint64_t i = (uint64_t)blockIdx.x * AS_TPB + threadIdx.x;
    if (i > R) return;
    st[i] = i ? ((uint64_t)nx[i] << 32) | i : 0;
}

// one pass in place: a 64-bit word is read and written whole, so a pair is consistent whichever pass made it
static __global__ void __launch_bounds__(AS_TPB) k_as_cyc_jump(uint64_t *st, uint64_t R, uint32_t *more) {
    const uint64_t i = (uint64_t)blockIdx.x * AS_TPB + threadIdx.x;
    uint32_t live = 0;
    if (i && i <= R) {
        const uint64_t v = __hip_atomic_load(st + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v >> 32) {
            const uint64_t u = __hip_atomic_load(st + (v >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t nv = (u & 0xFFFFFFFF00000000ull) | max((uint32_t)v, (uint32_t)u);
            __hip_atomic_store(st + i, nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            live = (nv >> 32) != 0;
        }
    }
    if (__any(live) && (threadIdx.x & 63) == 0) atomicOr(more, 1u);
}

// what still has a pointer lies on a cycle; the read that is its cycle's largest index cuts its link (:24-27)
static __global__ void __launch_bounds__(AS_TPB) k_as_cut(const uint64_t *__restrict__ st, uint64_t R, uint32_t *__restrict__ nx, uint16_t *__restrict__ ov,
                                                          uint32_t *__restrict__ pred, unsigned long long *__restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * AS_TPB + threadIdx.x;
    if (i == 0 || i > R) return;
    const uint64_t v = st[i];
    if (!(v >> 32) || (uint32_t)v != (uint32_t)i) return;
    atomicAdd(cnt + AS_CNT_CYCLES, 1ull);
    atomicAdd(cnt + AS_CNT_LOST, (unsigned long long)ov[i]);
    pred[nx[i]] = 0;
    nx[i] = 0;
    ov[i] = 0;
}

// st[i] = (pred[i], 1), a head points at itself with distance 0
static __global__ void __launch_bounds__(AS_TPB) k_as_rank_init(const uint32_t *__restrict__ pred, uint64_t R, uint64_t *__restrict__ st) {
    const uint64_t i = (uint64_t)blockIdx.x * AS_TPB + threadIdx.x;
    if (i > R) return;
    const uint32_t p = i ? pred[i] : 0;
    st[i] = p ? ((uint64_t)p << 32) | 1u : i << 32;
}

static __global__ void __launch_bounds__(AS_TPB) k_as_rank_jump(uint64_t *st, uint64_t R, uint32_t *more) {
    const uint64_t i = (uint64_t)blockIdx.x * AS_TPB + threadIdx.x;
    uint32_t live = 0;
    if (i && i <= R) {
        const uint64_t v = __hip_atomic_load(st + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t p = v >> 32;
        if (p != i) {
            const uint64_t u = __hip_atomic_load(st + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((u >> 32) != p) {       // p is no head yet: jump over it
                __hip_atomic_store(st + i, (u & 0xFFFFFFFF00000000ull) | (uint32_t)((uint32_t)v + (uint32_t)u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                live = 1;
            }
        }
    }
    if (__any(live) && (threadIdx.x & 63) == 0) atomicOr(more, 1u);
}

// a tail writes its chain's length at the head; heads are counted as components or singles
static __global__ void __launch_bounds__(AS_TPB) k_as_tails(const uint64_t *__restrict__ st, const uint32_t *__restrict__ nx, uint64_t R, uint32_t *__restrict__ len,
                                                            unsigned long long *__restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * AS_TPB + threadIdx.x;
    bool comp = false, single = false;
    if (i && i <= R) {
        const uint64_t v = st[i];
        const uint32_t n = nx[i];
        if (!n) len[v >> 32] = (uint32_t)v + 1u;
        if ((v >> 32) == i) {
            comp = n != 0;
            single = n == 0;
        }
    }
    const uint64_t bc = __ballot(comp), bs = __ballot(single);
    if ((threadIdx.x & 63) == 0) {
        if (bc) atomicAdd(cnt + AS_CNT_COMPONENTS, (unsigned long long)__popcll(bc));
        if (bs) atomicAdd(cnt + AS_CNT_SINGLES, (unsigned long long)__popcll(bs));
    }
}

// every read to its entry base[head] + distance: the walk order, the entry's shift, the NEXT entry's off, the original index
static __global__ void __launch_bounds__(AS_TPB) k_as_place(const uint64_t *__restrict__ st, const uint32_t *__restrict__ base, const uint16_t *__restrict__ ov,
                                                            const uint32_t *__restrict__ map, uint64_t R, uint32_t L, uint32_t *__restrict__ walk,
                                                            uint16_t *__restrict__ sh, uint16_t *__restrict__ off, uint32_t *__restrict__ org) {
    const uint64_t i = (uint64_t)blockIdx.x * AS_TPB + threadIdx.x;
    if (i == 0 || i > R) return;
    const uint64_t v = st[i];
    const uint64_t p = (uint64_t)base[v >> 32] + (uint32_t)v;
    if (p >= R) return;     // (a graph that passed the checks places every read below R)
    const uint16_t s = (uint16_t)(L - ov[i]);
    walk[p] = (uint32_t)i;
    sh[p] = s;
    if (p + 1 < R) off[p + 1] = s;
    if (p == 0) off[0] = 0;
    org[p] = map ? map[i - 1] : (uint32_t)(i - 1);
}

// first k in [lo, hi) with a[k] >= x (GREATER: > x), hi if none
template <bool GREATER>
__device__ __forceinline__ uint64_t as_bound(const uint64_t *__restrict__ a, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t v = a[mid];
        if (GREATER ? v <= x : v < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One tile of the text.  Entry j owns the bytes [start[j], start[j] + sh[j]): the tile's entries are j0 = the last one that
// starts at or before the tile (the one its first byte belongs to; entries of shift 0 that start there come before it) up to
// the first that starts at or after the tile's end.  A work item is AS_CHUNK row bytes of one entry, so long and short shifts
// load the threads alike; entries of shift 0 cost one look.  Every byte of [lo, hi) is written to LDS by exactly one item.
static __global__ void __launch_bounds__(AS_TPB) k_as_text(const uint8_t *__restrict__ rows, uint32_t rb, uint32_t symbols, const uint32_t *__restrict__ walk,
                                                           const uint16_t *__restrict__ sh, const uint64_t *__restrict__ start, uint64_t R, uint64_t pg_len,
                                                           uint8_t *__restrict__ text) {
    __shared__ uint4 tile4[AS_TILE / 16];
    __shared__ uint64_t s_j[2];
    uint8_t *tile = (uint8_t *)tile4;
    const uint64_t lo = (uint64_t)blockIdx.x * AS_TILE, hi = min(pg_len, lo + AS_TILE);
    for (uint32_t k = threadIdx.x; k < AS_TILE / 16; k += AS_TPB) tile4[k] = make_uint4(0, 0, 0, 0);
    if (threadIdx.x == 0) s_j[0] = as_bound<true>(start, 0, R, lo) - 1;     // start[0] = 0 <= lo
    if (threadIdx.x == 64) s_j[1] = as_bound<false>(start, 0, R, hi);
    __syncthreads();
    const uint64_t j0 = s_j[0], j1 = s_j[1];
    const bool five = symbols == 5;
    const uint32_t spb = five ? 3u : 4u, nch = (rb + AS_CHUNK - 1) / AS_CHUNK;
    const uint64_t items = (j1 - j0) * nch;
    for (uint64_t t = threadIdx.x; t < items; t += AS_TPB) {
        const uint64_t j = j0 + t / nch;
        const uint32_t c = (uint32_t)(t % nch), s = sh[j];
        if (c * AS_CHUNK * spb >= s) continue;
        const uint32_t r = walk[j];
        if (r == 0 || r > R) continue;      // (never for a graph that passed the checks: no row is read out of bounds)
        const uint8_t *row = rows + (uint64_t)(r - 1u) * rb;
        const uint64_t at = start[j];
        const uint32_t b1 = min(rb, (c + 1u) * AS_CHUNK);
        for (uint32_t b = c * AS_CHUNK; b < b1 && b * spb < s; b++) {
            const uint32_t v = row[b];
            for (uint32_t k = 0; k < spb; k++) {
                const uint32_t x = b * spb + k;
                const uint64_t pos = at + x;
                if (x < s && pos >= lo && pos < hi) {
                    const uint32_t code = five ? (k == 0 ? v / 25u : k == 1 ? (v / 5u) % 5u : v % 5u) : (v >> (6u - 2u * k)) & 3u;
                    tile[pos - lo] = as_ascii(code, five);
                }
            }
        }
    }
    __syncthreads();
    // whole lanes: the text buffer ends on a tile border, the bytes after pg_len are zero
    uint4 *dst = (uint4 *)(text + lo);
    for (uint32_t k = threadIdx.x; k < AS_TILE / 16; k += AS_TPB) dst[k] = tile4[k];
}

// ------------------------------------------------------------------------------------------------ host side
static int as_fail(pgrc_asm_ctx *a, const std::string &msg) { return dec_fail(a->d, PGRC_E_PARAM, "assemble: " + msg); }

// jumping passes until one reports no live pointer, `cap` at the most; *live_out: the last pass's report
static int as_jump(pgrc_asm_ctx *a, bool rank, uint64_t R, uint32_t cap, uint32_t *passes, uint32_t *live_out) {
    pgrc_decode_ctx *d = a->d;
    uint64_t *st = (uint64_t *)a->st.p;
    uint32_t *flag = (uint32_t *)d->flag.p, more = 1;
    int e;
    *passes = 0;
    while (more && *passes < cap) {
        if ((e = dec_clear_err(d))) return e;
        if (rank) hipLaunchKernelGGL(k_as_rank_jump, dim3(dec_grid(R + 1, AS_TPB)), dim3(AS_TPB), 0, d->stream, st, R, flag);
        else hipLaunchKernelGGL(k_as_cyc_jump, dim3(dec_grid(R + 1, AS_TPB)), dim3(AS_TPB), 0, d->stream, st, R, flag);
        HIP_TRY(d, hipGetLastError());
        HIP_TRY(d, hipMemcpyAsync(&more, flag, 4, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(d, hipStreamSynchronize(d->stream));
        ++*passes;
    }
    *live_out = more;
    return PGRC_OK;
}

// the input to the context's buffers: from the host, or (on_device: pgrc_ovl_assemble) rows, next_read and overlap from
// device memory of the same device; the index mapping is the caller's host array either way
static int as_stage(pgrc_asm_ctx *a, const pgrc_asm_input *in, bool on_device) {
    pgrc_decode_ctx *d = a->d;
    const uint64_t R = in->n_reads, N1 = R + 1;
    const uint32_t L = in->read_len, width = in->overlap_width;
    const uint32_t rb = in->symbols == 4 ? (L + 3) / 4 : (L + 2) / 3;
    int e;
    if (on_device) {
        HIP_TRY(d, hipMemcpyAsync(a->rows.p, in->packed_rows, R * rb, hipMemcpyDeviceToDevice, d->stream));
        HIP_TRY(d, hipMemcpyAsync(a->nx.p, in->next_read, N1 * 4, hipMemcpyDeviceToDevice, d->stream));
        HIP_TRY(d, hipMemcpyAsync(a->ovraw.p, in->overlap, N1 * width, hipMemcpyDeviceToDevice, d->stream));
    } else if ((e = dec_upload_host(d, a->rows.p, in->packed_rows, R * rb)) || (e = dec_upload_host(d, a->nx.p, in->next_read, N1 * 4)) ||
               (e = dec_upload_host(d, a->ovraw.p, in->overlap, N1 * width)))
        return e;
    if (in->index_mapping && (e = dec_upload_host(d, a->map.p, in->index_mapping, R * 4))) return e;
    return PGRC_OK;
}

// list_stays: the reads list is not brought down (pgasm_run_device_resident): out->org_idx and out->off stay NULL, the list
// lies in a->org and a->off for pgasm_last_list
static int as_run(pgrc_asm_ctx *a, const pgrc_asm_input *in, pgrc_asm_result *out, bool on_device, bool list_stays) {
    pgrc_decode_ctx *d = a->d;
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t R = in->n_reads, N1 = R + 1;
    const uint32_t L = in->read_len, symbols = in->symbols, width = in->overlap_width;
    const uint32_t rb = symbols == 4 ? (L + 3) / 4 : (L + 2) / 3;
    int e;
    if ((e = a->ev.ensure(d))) return e;
    const uint64_t fold_bytes = dec_a16(sco_scratch_elems(N1) * 8);
    if ((e = pgrc_bufs_unpooled(d, {{&a->rows, R * rb + 16}, {&a->nx, N1 * 4}, {&a->ovraw, N1 * width}, {&a->ov, N1 * 2}, {&a->pred, N1 * 4}, {&a->st, N1 * 8},
                                    {&a->len, N1 * 4}, {&a->walk, R * 4}, {&a->sh, R * 2}, {&a->off, R * 2}, {&a->org, R * 4}, {&a->start, N1 * 8},
                                    {&a->map, in->index_mapping ? R * 4 : 16}, {&a->fold, fold_bytes}, {&a->words, AS_BAD_WORDS * 4 + AS_CNT_WORDS * 8 + 16}})))
        return e;
    const uint8_t *rows = (const uint8_t *)a->rows.p;
    uint32_t *nx = (uint32_t *)a->nx.p, *pred = (uint32_t *)a->pred.p, *len = (uint32_t *)a->len.p, *walk = (uint32_t *)a->walk.p, *org = (uint32_t *)a->org.p;
    uint16_t *ov = (uint16_t *)a->ov.p, *sh = (uint16_t *)a->sh.p, *off = (uint16_t *)a->off.p;
    uint64_t *st = (uint64_t *)a->st.p, *start = (uint64_t *)a->start.p;
    const uint32_t *map = in->index_mapping ? (const uint32_t *)a->map.p : nullptr;
    unsigned long long *cnt = (unsigned long long *)a->words.p;
    uint32_t *bad = (uint32_t *)((uint8_t *)a->words.p + AS_CNT_WORDS * 8);

    if ((e = as_stage(a, in, on_device))) return e;
    HIP_TRY(d, hipMemsetAsync(nx, 0, 4, d->stream));            // element 0 is ignored: no successor
    HIP_TRY(d, hipMemsetAsync(pred, 0, N1 * 4, d->stream));
    HIP_TRY(d, hipMemsetAsync(len, 0, N1 * 4, d->stream));
    HIP_TRY(d, hipMemsetAsync(a->words.p, 0, AS_BAD_WORDS * 4 + AS_CNT_WORDS * 8, d->stream));
    const float ms_upload = dec_ms_since(t0);
    const uint32_t grid = dec_grid(N1, AS_TPB);

    // pred and the checks
    HIP_TRY(d, a->ev.record(0, d->stream));
    hipLaunchKernelGGL(k_as_pred, dim3(grid), dim3(AS_TPB), 0, d->stream, (const uint32_t *)nx, (const void *)a->ovraw.p, width, R, L, pred, ov, bad);
    hipLaunchKernelGGL(k_as_link, dim3(grid), dim3(AS_TPB), 0, d->stream, rows, rb, symbols, L, (const uint32_t *)nx, (const uint16_t *)ov, (const uint32_t *)pred, R, bad);
    if (symbols == 5) {
        const uint64_t total = R * rb;
        hipLaunchKernelGGL(k_as_rows5, dim3((uint32_t)std::min<uint64_t>(dec_grid(total, AS_TPB), 1u << 20)), dim3(AS_TPB), 0, d->stream, rows, total, rb, L, bad);
    }
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, a->ev.record(1, d->stream));
    uint32_t h_bad[AS_BAD_WORDS] = {};
    HIP_TRY(d, hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    // nothing below follows a pointer before the graph is known to be paths and cycles over 1 .. R
    if (h_bad[AS_BAD_NEXT]) return as_fail(a, "a successor above the reads' count " + std::to_string(R));
    if (h_bad[AS_BAD_PRED]) return as_fail(a, "a read has two predecessors");
    if (h_bad[AS_BAD_OVL]) return as_fail(a, "an overlap above the read length " + std::to_string(L));
    if (h_bad[AS_BAD_OVL_END]) return as_fail(a, "an overlap at a read without a successor");
    if (h_bad[AS_BAD_LINK]) return as_fail(a, "a link whose overlap is not real: the suffix of the read differs from the prefix of its successor");
    if (h_bad[AS_BAD_ROW]) return as_fail(a, "a row byte that is no packing of the alphabet");

    // cycles
    uint32_t bits = 0;
    while (bits < 33 && (1ull << bits) < N1) bits++;            // ceil(log2(R + 1))
    uint32_t passes_cyc = 0, passes_rank = 0, live = 0;
    HIP_TRY(d, a->ev.record(2, d->stream));
    hipLaunchKernelGGL(k_as_cyc_init, dim3(grid), dim3(AS_TPB), 0, d->stream, (const uint32_t *)nx, R, st);
    if ((e = as_jump(a, false, R, bits + 1, &passes_cyc, &live))) return e;
    if (live) hipLaunchKernelGGL(k_as_cut, dim3(grid), dim3(AS_TPB), 0, d->stream, (const uint64_t *)st, R, nx, ov, pred, cnt);
    HIP_TRY(d, hipGetLastError());

    // ranking
    HIP_TRY(d, a->ev.record(3, d->stream));
    hipLaunchKernelGGL(k_as_rank_init, dim3(grid), dim3(AS_TPB), 0, d->stream, (const uint32_t *)pred, R, st);
    if ((e = as_jump(a, true, R, bits + 3, &passes_rank, &live))) return e;
    if (live) return dec_fail(d, PGRC_E_DEVICE, "assemble: the chains did not resolve in " + std::to_string(passes_rank) + " passes");

    // lists
    HIP_TRY(d, a->ev.record(4, d->stream));
    hipLaunchKernelGGL(k_as_tails, dim3(grid), dim3(AS_TPB), 0, d->stream, (const uint64_t *)st, (const uint32_t *)nx, R, len, cnt);
    HIP_TRY(d, sco_scan<false>(d->stream, (const uint32_t *)len, len, N1, ScoIdentity{}, ScoPlus{}, 0u, (uint32_t *)a->fold.p));
    hipLaunchKernelGGL(k_as_place, dim3(grid), dim3(AS_TPB), 0, d->stream, (const uint64_t *)st, (const uint32_t *)len, (const uint16_t *)ov, map, R, L, walk, sh, off, org);
    HIP_TRY(d, sco_sum_u64<false>(d->stream, (const uint16_t *)sh, R, start, (uint64_t *)a->fold.p));
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, a->ev.record(5, d->stream));
    uint64_t pg_len = 0;
    unsigned long long h_cnt[AS_CNT_WORDS] = {};
    HIP_TRY(d, hipMemcpyAsync(&pg_len, start + R, 8, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipMemcpyAsync(h_cnt, cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    if (pg_len < L || pg_len > R * L) return dec_fail(d, PGRC_E_DEVICE, "assemble: a text of " + std::to_string(pg_len) + " symbols");

    // text: whole tiles, then the zero bytes the row kernels of a decode context expect after a text
    const uint64_t tiles = (pg_len + AS_TILE - 1) / AS_TILE;
    if ((e = pgrc_buf_unpooled(d, d->text, tiles * AS_TILE + DEC_TEXT_PAD))) return e;
    HIP_TRY(d, hipMemsetAsync((uint8_t *)d->text.p + tiles * AS_TILE, 0, DEC_TEXT_PAD, d->stream));
    hipLaunchKernelGGL(k_as_text, dim3((uint32_t)tiles), dim3(AS_TPB), 0, d->stream, rows, rb, symbols, (const uint32_t *)walk, (const uint16_t *)sh,
                       (const uint64_t *)start, R, pg_len, (uint8_t *)d->text.p);
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, a->ev.record(6, d->stream));

    // the reads list: one page-locked block, copied down while the text is made
    const auto t1 = std::chrono::steady_clock::now();
    const uint64_t off_at = dec_a16(R * 4), total = off_at + dec_a16(R * 2);
    uint8_t *blk = nullptr;
    float ms_download = 0;
    if (list_stays) {
        HIP_TRY(d, hipStreamSynchronize(d->stream));
    } else {
        hipError_t he = hipHostMalloc((void **)&blk, total);
        if (he != hipSuccess) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(d->stream);
            return dec_fail(d, PGRC_E_ALLOC, "assemble: hipHostMalloc(" + std::to_string(total) + ") failed");
        }
        he = hipMemcpyAsync(blk, org, R * 4, hipMemcpyDeviceToHost, d->copy_stream);
        if (he == hipSuccess) he = hipMemcpyAsync(blk + off_at, off, R * 2, hipMemcpyDeviceToHost, d->copy_stream);
        if (he == hipSuccess) he = hipStreamSynchronize(d->copy_stream);
        ms_download = dec_ms_since(t1);
        if (he == hipSuccess) he = hipStreamSynchronize(d->stream);
        if (he != hipSuccess) {
            (void)hipHostFree(blk);
            return dec_fail(d, pgrc_hip_code(he), std::string("assemble: copy down: ") + hipGetErrorString(he));
        }
    }
    out->struct_size = sizeof(pgrc_asm_result);
    out->pg_len = pg_len;
    out->n_reads = R;
    out->cycles = h_cnt[AS_CNT_CYCLES];
    out->overlap_lost = h_cnt[AS_CNT_LOST];
    out->components = h_cnt[AS_CNT_COMPONENTS];
    out->singles = h_cnt[AS_CNT_SINGLES];
    out->org_idx = (const uint32_t *)blk;
    out->off = blk ? (const uint16_t *)(blk + off_at) : nullptr;
    d->L = L;
    d->text_len = pg_len;
    d->have_text = true;
    a->symbols = symbols;
    a->list_n = R;
    a->list_mapped = map != nullptr;
    pgrc_asm_timing &t = a->tm;
    t = pgrc_asm_timing{};
    t.struct_size = sizeof(pgrc_asm_timing);
    t.passes_cycles = passes_cyc;
    t.passes_rank = passes_rank;
    t.ms_upload = ms_upload;
    t.ms_checks_device = a->ev.ms(0, 1);
    t.ms_cycles_device = a->ev.ms(2, 3);
    t.ms_rank_device = a->ev.ms(3, 4);
    t.ms_lists_device = a->ev.ms(4, 5);
    t.ms_text_device = a->ev.ms(5, 6);
    t.ms_download = ms_download;
    t.ms_call = dec_ms_since(t0);
    t.bytes_up = (on_device ? 0 : R * rb + N1 * 4 + N1 * width) + (map ? R * 4 : 0);
    t.bytes_down = list_stays ? 0 : R * 6;
    a->have_timing = true;
    return PGRC_OK;
}

static int as_entry(pgrc_asm_ctx *a, const pgrc_asm_input *in, pgrc_asm_result *out, bool on_device, bool list_stays = false) {
    if (!a) return PGRC_E_PARAM;
    if (!out) return as_fail(a, "out is NULL");
    *out = pgrc_asm_result{};
    // the last run's text goes whatever becomes of this one
    a->d->have_text = false;
    a->d->have_parts = false;
    a->d->nl = 0;
    a->d->have_order = false;
    a->have_packed = false;
    a->have_timing = false;
    if (!in) return as_fail(a, "in is NULL");
    if (in->struct_size != sizeof(pgrc_asm_input)) return as_fail(a, "struct_size is not sizeof(pgrc_asm_input)");
    if (in->read_len < 1 || in->read_len > 255) return as_fail(a, "the read length must be in [1, 255]");
    if (in->symbols != 4 && in->symbols != 5) return as_fail(a, "the alphabet has 4 (ACGT) or 5 (ACGNT) symbols");
    if (in->overlap_width != 1 && in->overlap_width != 2) return as_fail(a, "an overlap has 1 or 2 bytes");
    if (in->n_reads < 1 || in->n_reads > 0xFFFFFFFEull) return as_fail(a, "the reads' count must be in [1, 2^32 - 2]");
    if (!in->packed_rows || !in->next_read || !in->overlap) return as_fail(a, "packed_rows, next_read or overlap is NULL");
    PGRC_ON_DEVICE(a->d);
    const int e = as_run(a, in, out, on_device, list_stays);
    if (e) {
        (void)hipStreamSynchronize(a->d->stream);
        *out = pgrc_asm_result{};
    }
    return e;
}

int pgasm_run_device(pgrc_asm_ctx *a, const pgrc_asm_input *in, pgrc_asm_result *out) { return as_entry(a, in, out, true); }
int pgasm_run_device_resident(pgrc_asm_ctx *a, const pgrc_asm_input *in, pgrc_asm_result *out) { return as_entry(a, in, out, true, true); }
int pgasm_device(const pgrc_asm_ctx *a) { return a->d->device; }

void pgasm_last_list(const pgrc_asm_ctx *a, PgasmLastList *out) {
    *out = PgasmLastList{};
    out->device = a->d->device;
    out->valid = a->d->have_text;
    if (!out->valid) return;
    out->mapped = a->list_mapped;
    out->n = a->list_n;
    out->read_len = a->d->L;
    out->pg_len = a->d->text_len;
    out->d_org = (const uint32_t *)a->org.p;
    out->d_off = (const uint16_t *)a->off.p;
}

extern "C" {

int pgrc_asm_create(int32_t device, pgrc_asm_ctx **out) {
    if (!out) return PGRC_E_PARAM;
    *out = nullptr;
    pgrc_decode_ctx *d = nullptr;
    const int e = pgrc_decode_create_on(device, &d);
    if (e) return e;
    pgrc_asm_ctx *a = new pgrc_asm_ctx();
    a->d = d;
    *out = a;
    return PGRC_OK;
}

void pgrc_asm_destroy(pgrc_asm_ctx *a) {
    if (!a) return;
    {
        PgrcDeviceScope scope(a->d->device);
        (void)hipStreamSynchronize(a->d->stream);
        dec_free_all(as_bufs(a));
        a->ev.release();
    }
    pgrc_decode_destroy(a->d);
    delete a;
}

const char *pgrc_asm_last_error(const pgrc_asm_ctx *a) { return pgrc_decode_last_error(a ? a->d : nullptr); }

int pgrc_asm_run(pgrc_asm_ctx *a, const pgrc_asm_input *in, pgrc_asm_result *out) { return as_entry(a, in, out, false); }

void pgrc_asm_free_result(pgrc_asm_result *r) {
    if (!r) return;
    if (r->org_idx) (void)hipHostFree(const_cast<uint32_t *>(r->org_idx));
    *r = pgrc_asm_result{};
}

int pgrc_asm_get_text(pgrc_asm_ctx *a, uint64_t first, uint64_t n, char *out) {
    if (!a) return PGRC_E_PARAM;
    return pgrc_decode_get_text(a->d, first, n, out);
}

int pgrc_asm_text_device(pgrc_asm_ctx *a, const void **d_ascii, uint64_t *len) {
    if (!a) return PGRC_E_PARAM;
    if (!d_ascii || !len) return as_fail(a, "d_ascii or len is NULL");
    if (!a->d->have_text) return dec_fail(a->d, PGRC_E_STATE, "assemble: no run has succeeded on this context");
    *d_ascii = a->d->text.p;
    *len = a->d->text_len;
    return PGRC_OK;
}

int pgrc_asm_packed_device(pgrc_asm_ctx *a, const void **d_words) {
    if (!a) return PGRC_E_PARAM;
    if (!d_words) return as_fail(a, "d_words is NULL");
    *d_words = nullptr;
    pgrc_decode_ctx *d = a->d;
    if (!d->have_text) return dec_fail(d, PGRC_E_STATE, "assemble: no run has succeeded on this context");
    if (a->symbols != 4) return as_fail(a, "the 2-bit text exists over ACGT only");
    PGRC_ON_DEVICE(d);
    if (!a->have_packed) {
        const uint64_t nwords = (d->text_len + 15) / 16;
        int e;
        if ((e = pgrc_buf_unpooled(d, a->packed, nwords * 4 + 64))) return e;
        if ((e = dec_clear_err(d))) return e;
        HIP_TRY(d, hipMemsetAsync((uint32_t *)a->packed.p + nwords, 0, 64, d->stream));
        if ((e = pgrc_launch_pack_ascii(d, d->stream, (const uint8_t *)d->text.p, d->text_len, (uint32_t *)a->packed.p, (uint32_t *)d->flag.p)))
            return dec_fail(d, e, "assemble: " + d->err);
        uint32_t symerr = 0;
        HIP_TRY(d, hipMemcpyAsync(&symerr, d->flag.p, 4, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(d, hipStreamSynchronize(d->stream));
        if (symerr) return dec_fail(d, PGRC_E_DEVICE, "assemble: the text holds a byte outside ACGT");
        a->have_packed = true;
    }
    *d_words = a->packed.p;
    return PGRC_OK;
}

int pgrc_asm_get_timing(pgrc_asm_ctx *a, pgrc_asm_timing *out) {
    if (!a) return PGRC_E_PARAM;
    if (!out || out->struct_size != sizeof(pgrc_asm_timing)) return dec_fail(a->d, PGRC_E_PARAM, "timing is NULL or struct_size is not sizeof(pgrc_asm_timing)");
    if (!a->have_timing) return dec_fail(a->d, PGRC_E_STATE, "assemble: no run has succeeded on this context");
    *out = a->tm;
    return PGRC_OK;
}

}   // extern "C"
