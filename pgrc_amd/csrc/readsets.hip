// readsets.hip -- the divided read sets of the encoder on the device (include/pgrc_readsets.h): the
// DividedPCLReadsSets object (readsset/DividedPCLReadsSets.cpp) -- the packed HQ, LQ and N sets and the two index mappings -- and
// its four edits between the encoder's stages: moveLqReadsFromHqReadsSetsToLqReadsSets (:145-197), generateHqReadsIndexesMapping
// (:199-216), removeReadsFromLqReadsSet and removeReadsFromNReadsSet (:218-246).
//
// The reference walks all reads in a serial loop with a copyRead per row.  Here every edit works on the original indexes 0 .. A - 1:
//   classes      one byte per original index: 0 (HQ), 1 at the LQ mapping's entries, 2 at the N mapping's.  Every entry reads back
//                its own class (so no index is in both lists), is below A and above the entry before it
//   counts       exclusive counts of the classes over the indexes (scanops.h): class 1 counts the old LQ rows, class 0 the old HQ
//                rows.  A move turns the HQ indexes whose flag is 0 into class 3 and counts those too
//   descriptors  every output row gets one u32: its source row, the source set in the top bit.  New LQ set: classes {1, 3} in
//                ascending index; new HQ set: class 0.  A removal is the same over the rows of one set: the rows whose flag is 0
//   rows         ONE kernel for all edits: output row r is source row desc[r] of one of two arrays (k_rs_rows below)
// Edits are out of place: the new buffers replace the old ones when the call has succeeded.  No library kernel, no global atomic.
#include <chrono>
#include <vector>

#include "devutil.h"
#include "rsetsctx.h"

#define RS_TPB 256
#define RS_TILE_BYTES 12288u        // the LDS image of a tile of output rows
#define RS_SRC1 0x80000000u         // a descriptor's top bit: the row comes from the second source array

// the words of `words`: the refusals of the checks, then the totals of the counts
enum { RS_BAD_RANGE, RS_BAD_ASCEND, RS_BAD_BOTH, RS_BAD_WORDS };

static thread_local std::string g_rs_create_err;

static int rs_fail(pgrc_rsets *s, int code, const std::string &msg) { return dec_fail(s, code, "read sets: " + msg); }

static DevBufList rs_bufs(pgrc_rsets *s) {
    DevBufList all = {&s->cls, &s->cnt[0], &s->cnt[1], &s->cnt[2], &s->flags, &s->desc[0], &s->desc[1], &s->fold, &s->words, &s->stage_idx};
    for (RsSet &t : s->set) all.insert(all.end(), {&t.rows, &t.map});
    return all;
}

// ------------------------------------------------------------------------------------------------ kernels: classes and counts
static __global__ void __launch_bounds__(RS_TPB) k_rs_offset(const uint32_t *__restrict__ in, uint64_t n, uint32_t base, uint32_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * RS_TPB + threadIdx.x;
    if (i < n) out[i] = in[i] + base;
}

static __global__ void __launch_bounds__(RS_TPB) k_rs_scatter(const uint32_t *__restrict__ map, uint64_t n, uint64_t A, uint8_t c, uint8_t *__restrict__ cls) {
    const uint64_t i = (uint64_t)blockIdx.x * RS_TPB + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = map[i];
    if (v < A) cls[v] = c;
}

// every entry reads back its own class: an index that is in both lists has lost its class of one of them
static __global__ void __launch_bounds__(RS_TPB) k_rs_check(const uint32_t *__restrict__ map, uint64_t n, uint64_t A, uint8_t c, const uint8_t *__restrict__ cls,
                                                            uint32_t *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * RS_TPB + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = map[i];
    if (v >= A) bad[RS_BAD_RANGE] = 1;
    else if (cls[v] != c) bad[RS_BAD_BOTH] = 1;
    if (i && map[i - 1] >= v) bad[RS_BAD_ASCEND] = 1;
}

struct RsIsClass {      // 1 where the class is c
    const uint8_t *cls;
    uint8_t c;
    __device__ uint32_t operator()(uint64_t i) const { return cls[i] == c ? 1u : 0u; }
};
struct RsIsZero {       // 1 where the flag is 0: a row that stays
    const uint8_t *f;
    __device__ uint32_t operator()(uint64_t i) const { return f[i] ? 0u : 1u; }
};

// the move: an HQ index whose flag is 0 becomes class 3 (hq[a] = the HQ rows in front of index a)
// nh: the flags' count; the host has made sure that it is the class-0 count, the bound keeps a read inside the array regardless
static __global__ void __launch_bounds__(RS_TPB) k_rs_mark_moved(uint8_t *__restrict__ cls, uint64_t A, const uint32_t *__restrict__ hq, const uint8_t *__restrict__ is_hq, uint64_t nh) {
    const uint64_t a = (uint64_t)blockIdx.x * RS_TPB + threadIdx.x;
    if (a < A && cls[a] == 0 && hq[a] < nh && !is_hq[hq[a]]) cls[a] = 3;
}

// ------------------------------------------------------------------------------------------------ kernels: descriptors
// hq / lq / mv: the old HQ rows, the old LQ rows and the moved rows in front of index a (element A: the totals)
static __global__ void __launch_bounds__(RS_TPB) k_rs_move_desc(const uint8_t *__restrict__ cls, uint64_t A, const uint32_t *__restrict__ hq, const uint32_t *__restrict__ lq,
                                                                const uint32_t *__restrict__ mv, uint32_t *__restrict__ desc_lq, uint32_t *__restrict__ map_lq,
                                                                uint32_t *__restrict__ desc_hq) {
    const uint64_t a = (uint64_t)blockIdx.x * RS_TPB + threadIdx.x;
    if (a > A) return;
    if (a == A) {
        map_lq[lq[A] + mv[A]] = (uint32_t)A;        // the guard
        return;
    }
    const uint32_t c = cls[a];
    if (c == 1 || c == 3) {
        const uint32_t p = lq[a] + mv[a];
        desc_lq[p] = c == 1 ? lq[a] : (hq[a] | RS_SRC1);
        map_lq[p] = (uint32_t)a;
    } else if (c == 0) {
        desc_hq[hq[a] - mv[a]] = hq[a];
    }
}

// a removal: the rows whose flag is 0, in order (at[i] = such rows in front of row i, at[n] = their count)
static __global__ void __launch_bounds__(RS_TPB) k_rs_keep_desc(const uint8_t *__restrict__ flags, uint64_t n, const uint32_t *__restrict__ at, const uint32_t *__restrict__ map_old,
                                                                uint32_t guard, uint32_t *__restrict__ desc, uint32_t *__restrict__ map_new) {
    const uint64_t i = (uint64_t)blockIdx.x * RS_TPB + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        map_new[at[n]] = guard;
        return;
    }
    if (!flags[i]) {
        desc[at[i]] = (uint32_t)i;
        map_new[at[i]] = map_old[i];
    }
}

// generateHqReadsIndexesMapping: the class-0 indexes in ascending order, the guard behind them
static __global__ void __launch_bounds__(RS_TPB) k_rs_hq_map(const uint8_t *__restrict__ cls, uint64_t A, const uint32_t *__restrict__ hq, uint32_t *__restrict__ out) {
    const uint64_t a = (uint64_t)blockIdx.x * RS_TPB + threadIdx.x;
    if (a > A) return;
    if (a == A) out[hq[A]] = (uint32_t)A;
    else if (cls[a] == 0) out[hq[a]] = (uint32_t)a;
}

static __global__ void __launch_bounds__(RS_TPB) k_rs_matched(const uint64_t *__restrict__ pos, uint64_t n, uint8_t *__restrict__ flags) {
    const uint64_t i = (uint64_t)blockIdx.x * RS_TPB + threadIdx.x;
    if (i < n) flags[i] = pos[i] != PGRC_NOT_MATCHED_POS;
}

// ------------------------------------------------------------------------------------------------ the row mover
struct RsSrc {
    const uint8_t *p[2];        // two source arrays of rows (hipMalloc'ed: at least 4-byte aligned), without a pad
    uint64_t rows[2];
};

// the aligned dword at byte `a` of an array of `size` bytes; where the array ends inside it, only the bytes it has
__device__ __forceinline__ uint32_t rs_ld(const uint8_t *__restrict__ base, uint64_t size, uint64_t a) {
    if (a + 4 <= size) return *reinterpret_cast<const uint32_t *>(base + a);
    uint32_t w = 0;
    for (uint32_t k = 0; k < 4 && a + k < size; k++) w |= (uint32_t)base[a + k] << (8u * k);
    return w;
}

// Output row r (rb bytes, 1 .. 85, mostly no multiple of 4) is source row desc[r] of src.p[desc[r] >> 31].  A block takes a tile of
// tile_rows output rows -- a multiple of 16, so the tile's bytes start 16-byte aligned in `out` -- and builds its image in LDS:
// lane after lane takes the next dword of the image, finds the row (or the two to four rows) it lies in and fetches its bytes
// with aligned dword loads and a funnel shift.  The moves are compactions and merges: inside a source set the rows of a tile
// ascend and are mostly neighbours, so neighbouring lanes read neighbouring dwords and a wave's loads fall into few lines.  The
// image then goes out in whole 16-byte stores.  The last tile ends with the array: its last bytes go out one by one, and no
// load touches a byte behind a source array's end (rs_ld).  magic = floor(2^32 / rb) + 1: byte / rb for the bytes of a tile.
static __global__ void __launch_bounds__(RS_TPB) k_rs_rows(RsSrc src, const uint32_t *__restrict__ desc, uint64_t nout, uint32_t rb, uint32_t magic, uint32_t tile_rows,
                                                           uint8_t *__restrict__ out) {
    __shared__ uint4 img4[RS_TILE_BYTES / 16];
    uint32_t *img = reinterpret_cast<uint32_t *>(img4);
    const uint64_t r0 = (uint64_t)blockIdx.x * tile_rows;
    if (r0 >= nout) return;
    const uint32_t rows = (uint32_t)min((uint64_t)tile_rows, nout - r0);
    const uint32_t nbytes = rows * rb, ndw = (nbytes + 3u) / 4u;
    for (uint32_t w = threadIdx.x; w < ndw; w += RS_TPB) {
        const uint32_t b = 4u * w;
        uint32_t val = 0, k = 0;
        while (k < 4u && b + k < nbytes) {
            const uint32_t x = b + k;
            const uint32_t row = rb == 1u ? x : __umulhi(x, magic);
            const uint32_t off = x - row * rb;
            const uint32_t len = min(4u - k, rb - off);
            const uint32_t ds = desc[r0 + row], set = ds >> 31, sr = ds & ~RS_SRC1;
            uint32_t piece = 0;
            if (sr < src.rows[set]) {
                const uint8_t *base = src.p[set];
                const uint64_t size = src.rows[set] * rb, s = (uint64_t)sr * rb + off, a = s & ~3ull;
                const uint32_t in = (uint32_t)(s & 3u);
                const uint32_t lo = rs_ld(base, size, a);
                const uint32_t hi = in + len > 4u ? rs_ld(base, size, a + 4) : 0u;      // (the row's bytes reach into it: it begins inside the array)
                piece = funnel_r(lo, hi, 8u * in);
                if (len < 4u) piece &= (1u << (8u * len)) - 1u;
            }
            val |= piece << (8u * k);
            k += len;
        }
        img[w] = val;
    }
    __syncthreads();
    uint8_t *o = out + r0 * rb;
    const uint32_t n16 = nbytes / 16u;
    for (uint32_t q = threadIdx.x; q < n16; q += RS_TPB) reinterpret_cast<uint4 *>(o)[q] = img4[q];
    const uint8_t *img1 = reinterpret_cast<const uint8_t *>(img4);
    for (uint32_t t = n16 * 16u + threadIdx.x; t < nbytes; t += RS_TPB) o[t] = img1[t];
}

// ------------------------------------------------------------------------------------------------ host side: helpers
static int rs_move_rows(pgrc_rsets *s, const uint8_t *src0, uint64_t n0, const uint8_t *src1, uint64_t n1, const uint32_t *desc, uint64_t nout, uint32_t rb, uint8_t *out) {
    if (!nout || !rb) return PGRC_OK;
    RsSrc src;
    src.p[0] = src0; src.rows[0] = n0;
    src.p[1] = src1; src.rows[1] = n1;
    const uint32_t tile_rows = std::max(16u, (RS_TILE_BYTES / rb) & ~15u);
    const uint32_t magic = rb == 1 ? 0u : (uint32_t)((1ull << 32) / rb) + 1u;
    const uint64_t tiles = (nout + tile_rows - 1) / tile_rows;
    hipLaunchKernelGGL(k_rs_rows, dim3((uint32_t)tiles), dim3(RS_TPB), 0, s->stream, src, desc, nout, rb, magic, tile_rows, out);
    HIP_TRY(s, hipGetLastError());
    s->tm.rows_moved += nout;
    s->tm.bytes_moved += nout * rb;
    return PGRC_OK;
}

// what a set holds into its new, larger buffer; the new buffer is given back if the copy fails
static int rs_copy_kept(PgrcStage *s, DevBuf &nb, const void *old, uint64_t bytes) {
    hipError_t he = bytes ? hipMemcpyAsync(nb.p, old, bytes, hipMemcpyDeviceToDevice, s->stream) : hipSuccess;
    if (he == hipSuccess) he = hipStreamSynchronize(s->stream);
    if (he == hipSuccess) return PGRC_OK;
    dec_free(nb);
    return dec_fail(s, pgrc_hip_code(he), std::string("read sets: growing a set: ") + hipGetErrorString(he));
}

// room for `rows` rows / `entries` mapping entries, what the set holds kept
static int rs_reserve(pgrc_rsets *s, RsSet &t, uint64_t rows, uint64_t entries) {
    int e;
    if (rows > t.cap_rows) {
        const uint64_t cap = std::max(rows, t.cap_rows * 2);
        DevBuf nb;
        if ((e = pgrc_buf_unpooled(s, nb, cap * t.rb))) return e;
        if ((e = rs_copy_kept(s, nb, t.rows.p, t.n * t.rb))) return e;
        dec_free(t.rows);
        t.rows = nb;
        t.cap_rows = cap;
    }
    if (entries > t.cap_map) {
        const uint64_t cap = std::max(entries, t.cap_map * 2);
        DevBuf nb;
        if ((e = pgrc_buf_unpooled(s, nb, cap * 4))) return e;
        if ((e = rs_copy_kept(s, nb, t.map.p, t.n * 4))) return e;
        dec_free(t.map);
        t.map = nb;
        t.cap_map = cap;
    }
    return PGRC_OK;
}

static int rs_bad_words(pgrc_rsets *s, const uint32_t *bad, const char *what) {
    if (bad[RS_BAD_RANGE]) return rs_fail(s, PGRC_E_PARAM, std::string(what) + ": an index at or above the reads' count");
    if (bad[RS_BAD_ASCEND]) return rs_fail(s, PGRC_E_PARAM, std::string(what) + ": a mapping does not ascend strictly");
    if (bad[RS_BAD_BOTH]) return rs_fail(s, PGRC_E_PARAM, std::string(what) + ": an index is in both mappings");
    return PGRC_OK;
}

// the class bytes of `A` indexes from two lists (either may be empty) and their checks, queued; `bad` cleared first
static int rs_classes_of(pgrc_rsets *s, uint64_t A, const uint32_t *lq, uint64_t nl, const uint32_t *nn_map, uint64_t nn) {
    int e;
    if ((e = pgrc_bufs_unpooled(s, {{&s->cls, A + 16}, {&s->words, 64}}))) return e;
    uint8_t *cls = (uint8_t *)s->cls.p;
    uint32_t *bad = (uint32_t *)s->words.p;
    if (A) HIP_TRY(s, hipMemsetAsync(cls, 0, A, s->stream));
    HIP_TRY(s, hipMemsetAsync(bad, 0, 64, s->stream));
    if (nl) hipLaunchKernelGGL(k_rs_scatter, dim3(dec_grid(nl, RS_TPB)), dim3(RS_TPB), 0, s->stream, lq, nl, A, (uint8_t)1, cls);
    if (nn) hipLaunchKernelGGL(k_rs_scatter, dim3(dec_grid(nn, RS_TPB)), dim3(RS_TPB), 0, s->stream, nn_map, nn, A, (uint8_t)2, cls);
    if (nl) hipLaunchKernelGGL(k_rs_check, dim3(dec_grid(nl, RS_TPB)), dim3(RS_TPB), 0, s->stream, lq, nl, A, (uint8_t)1, (const uint8_t *)cls, bad);
    if (nn) hipLaunchKernelGGL(k_rs_check, dim3(dec_grid(nn, RS_TPB)), dim3(RS_TPB), 0, s->stream, nn_map, nn, A, (uint8_t)2, (const uint8_t *)cls, bad);
    HIP_TRY(s, hipGetLastError());
    return PGRC_OK;
}
static int rs_classes(pgrc_rsets *s) {
    return rs_classes_of(s, s->A, (const uint32_t *)s->set[1].map.p, s->set[1].n, (const uint32_t *)s->set[2].map.p, s->set[2].n);
}

// cnt[k][0 .. n] = the exclusive counts of `in`, element n the total
template <typename In>
static int rs_count(pgrc_rsets *s, In in, uint64_t n, int k) {
    int e;
    if ((e = pgrc_bufs_unpooled(s, {{&s->cnt[k], (n + 1) * 4}, {&s->fold, sco_scratch_elems(n + 1) * 4 + 16}}))) return e;
    HIP_TRY(s, (sco_device_scan<false, true>(s->stream, in, n, ScoPlus{}, 0u, 0u, ScoStore<uint32_t>{(uint32_t *)s->cnt[k].p}, (uint32_t *)s->fold.p)));
    return PGRC_OK;
}

// the flags of an edit on the device: the caller's device pointer, or its host bytes uploaded
static int rs_flags(pgrc_rsets *s, const uint8_t *flags, uint64_t n, int32_t on_device, const uint8_t **d_flags) {
    if (on_device || !n) { *d_flags = flags; return PGRC_OK; }
    int e;
    if ((e = pgrc_buf_unpooled(s, s->flags, n + 16)) || (e = dec_upload_host(s, s->flags.p, flags, n))) return e;
    *d_flags = (const uint8_t *)s->flags.p;
    return PGRC_OK;
}

// a move needs the HQ set to hold every read that is in neither mapping: after a removal it no longer does (the removed reads
// are in neither), and the flags' array has one byte per HQ row, not per such read.  Known on the host: asked before any launch.
static int rs_move_allowed(pgrc_rsets *s) {
    if (s->prm.n_reads_lq) return rs_fail(s, PGRC_E_PARAM, "move: the HQ and the LQ set are packed with different alphabets (n_reads_lq)");
    if (s->set[0].n != s->A - s->set[1].n - s->set[2].n)
        return rs_fail(s, PGRC_E_PARAM, "move: the HQ count is not the reads' count minus the LQ and N counts (after a removal the HQ set no longer holds every read in neither mapping)");
    if (s->set[0].n >= 0x80000000ull || s->set[1].n >= 0x80000000ull) return rs_fail(s, PGRC_E_PARAM, "move: a set of 2^31 rows or more");
    return PGRC_OK;
}

static int rs_need(pgrc_rsets *s, const char *what, std::initializer_list<int> sets) {
    if (!s->finished) return rs_fail(s, PGRC_E_STATE, std::string(what) + " before pgrc_rsets_finish");
    for (int k : sets)
        if (s->set[k].disposed) return rs_fail(s, PGRC_E_STATE, std::string(what) + ": the " + (k == 0 ? "HQ" : k == 1 ? "LQ" : "N") + " set has been disposed");
    return PGRC_OK;
}

// ------------------------------------------------------------------------------------------------ host side: the edits
static int rs_move(pgrc_rsets *s, const uint8_t *d_is_hq) {
    const auto t0 = std::chrono::steady_clock::now();
    RsSet &hq = s->set[0], &lq = s->set[1];
    const uint64_t A = s->A, nh = hq.n, nl = lq.n;
    const uint32_t rb = hq.rb;
    int e;
    if ((e = s->ev.ensure(s))) return e;
    s->tm = pgrc_rsets_timing{};
    s->have_timing = false;
    HIP_TRY(s, s->ev.record(0, s->stream));
    if ((e = rs_classes(s))) return e;
    uint8_t *cls = (uint8_t *)s->cls.p;
    if ((e = rs_count(s, RsIsClass{cls, 0}, A, 0)) || (e = rs_count(s, RsIsClass{cls, 1}, A, 1))) return e;
    const uint32_t *c_hq = (const uint32_t *)s->cnt[0].p, *c_lq = (const uint32_t *)s->cnt[1].p;
    if (A) hipLaunchKernelGGL(k_rs_mark_moved, dim3(dec_grid(A, RS_TPB)), dim3(RS_TPB), 0, s->stream, cls, A, c_hq, d_is_hq, nh);
    HIP_TRY(s, hipGetLastError());
    if ((e = rs_count(s, RsIsClass{cls, 3}, A, 2))) return e;
    const uint32_t *c_mv = (const uint32_t *)s->cnt[2].p;
    HIP_TRY(s, s->ev.record(1, s->stream));
    uint32_t bad[RS_BAD_WORDS] = {}, tot[3] = {};
    HIP_TRY(s, hipMemcpyAsync(bad, s->words.p, sizeof bad, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipMemcpyAsync(&tot[0], c_hq + A, 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipMemcpyAsync(&tot[1], c_lq + A, 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipMemcpyAsync(&tot[2], c_mv + A, 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    if ((e = rs_bad_words(s, bad, "move"))) return e;
    if (tot[0] != nh || tot[1] != nl || tot[2] > nh) return rs_fail(s, PGRC_E_PARAM, "move: the HQ count is not the reads' count minus the LQ and N counts");
    const uint64_t moved = tot[2], new_nl = nl + moved, new_nh = nh - moved;
    DevBuf n_lq_rows, n_lq_map, n_hq_rows;
    auto drop = [&]() { dec_free(n_lq_rows); dec_free(n_lq_map); dec_free(n_hq_rows); };
    if ((e = pgrc_bufs_unpooled(s, {{&n_lq_rows, new_nl * rb}, {&n_lq_map, (new_nl + 1) * 4}, {&n_hq_rows, new_nh * rb}, {&s->desc[0], new_nl * 4}, {&s->desc[1], new_nh * 4}}))) {
        drop();
        return e;
    }
    hipError_t he = hipSuccess;
    hipLaunchKernelGGL(k_rs_move_desc, dim3(dec_grid(A + 1, RS_TPB)), dim3(RS_TPB), 0, s->stream, (const uint8_t *)cls, A, c_hq, c_lq, c_mv, (uint32_t *)s->desc[0].p, (uint32_t *)n_lq_map.p,
                       (uint32_t *)s->desc[1].p);
    he = hipGetLastError();
    if (he == hipSuccess) he = s->ev.record(2, s->stream);
    if (he == hipSuccess) {
        e = rs_move_rows(s, (const uint8_t *)lq.rows.p, nl, (const uint8_t *)hq.rows.p, nh, (const uint32_t *)s->desc[0].p, new_nl, rb, (uint8_t *)n_lq_rows.p);
        if (!e) e = rs_move_rows(s, (const uint8_t *)hq.rows.p, nh, (const uint8_t *)hq.rows.p, nh, (const uint32_t *)s->desc[1].p, new_nh, rb, (uint8_t *)n_hq_rows.p);
        if (e) { (void)hipStreamSynchronize(s->stream); drop(); return e; }
        he = s->ev.record(3, s->stream);
    }
    if (he == hipSuccess) he = hipStreamSynchronize(s->stream);
    if (he != hipSuccess) {
        drop();
        return rs_fail(s, pgrc_hip_code(he), std::string("move: ") + hipGetErrorString(he));
    }
    dec_free(lq.rows); dec_free(lq.map); dec_free(hq.rows);
    lq.rows = n_lq_rows; lq.map = n_lq_map; hq.rows = n_hq_rows;
    lq.n = new_nl; lq.cap_rows = new_nl; lq.cap_map = new_nl + 1;
    hq.n = new_nh; hq.cap_rows = new_nh;
    s->hq_gen++;
    s->tm.struct_size = sizeof(pgrc_rsets_timing);
    s->tm.edit = 1;
    s->tm.ms_checks_device = s->ev.ms(0, 1);
    s->tm.ms_desc_device = s->ev.ms(1, 2);
    s->tm.ms_rows_device = s->ev.ms(2, 3);
    s->tm.ms_call = dec_ms_since(t0);
    s->have_timing = true;
    return PGRC_OK;
}

static int rs_remove(pgrc_rsets *s, const uint8_t *d_flags) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t A = s->A;
    const bool have_n = s->set[2].symbols != 0;
    const int last = have_n ? 2 : 1;
    int e;
    if ((e = s->ev.ensure(s))) return e;
    s->tm = pgrc_rsets_timing{};
    s->have_timing = false;
    HIP_TRY(s, s->ev.record(0, s->stream));
    const uint8_t *f[3] = {nullptr, d_flags, d_flags + s->set[1].n};        // nBegIdx: the LQ count before its removal
    for (int k = 1; k <= last; k++)
        if ((e = rs_count(s, RsIsZero{f[k]}, s->set[k].n, k - 1))) return e;
    HIP_TRY(s, s->ev.record(1, s->stream));
    uint32_t kept[3] = {};
    for (int k = 1; k <= last; k++) HIP_TRY(s, hipMemcpyAsync(&kept[k], (const uint32_t *)s->cnt[k - 1].p + s->set[k].n, 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    DevBuf n_rows[3], n_map[3];
    auto drop = [&]() { for (int k = 1; k <= 2; k++) { dec_free(n_rows[k]); dec_free(n_map[k]); } };
    for (int k = 1; k <= last; k++) {
        RsSet &t = s->set[k];
        if (kept[k] > t.n) { drop(); return rs_fail(s, PGRC_E_DEVICE, "remove: more rows kept than the set holds"); }
        if ((e = pgrc_bufs_unpooled(s, {{&n_rows[k], (uint64_t)kept[k] * t.rb}, {&n_map[k], ((uint64_t)kept[k] + 1) * 4}, {&s->desc[k - 1], (uint64_t)kept[k] * 4}}))) {
            drop();
            return e;
        }
        hipLaunchKernelGGL(k_rs_keep_desc, dim3(dec_grid(t.n + 1, RS_TPB)), dim3(RS_TPB), 0, s->stream, f[k], t.n, (const uint32_t *)s->cnt[k - 1].p, (const uint32_t *)t.map.p, (uint32_t)A,
                           (uint32_t *)s->desc[k - 1].p, (uint32_t *)n_map[k].p);
    }
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = s->ev.record(2, s->stream);
    for (int k = 1; k <= last && he == hipSuccess; k++) {
        RsSet &t = s->set[k];
        if ((e = rs_move_rows(s, (const uint8_t *)t.rows.p, t.n, (const uint8_t *)t.rows.p, t.n, (const uint32_t *)s->desc[k - 1].p, kept[k], t.rb, (uint8_t *)n_rows[k].p))) {
            (void)hipStreamSynchronize(s->stream);
            drop();
            return e;
        }
    }
    if (he == hipSuccess) he = s->ev.record(3, s->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(s->stream);
    if (he != hipSuccess) {
        drop();
        return rs_fail(s, pgrc_hip_code(he), std::string("remove: ") + hipGetErrorString(he));
    }
    for (int k = 1; k <= last; k++) {
        RsSet &t = s->set[k];
        dec_free(t.rows); dec_free(t.map);
        t.rows = n_rows[k]; t.map = n_map[k];
        t.n = kept[k]; t.cap_rows = kept[k]; t.cap_map = (uint64_t)kept[k] + 1;
    }
    s->tm.struct_size = sizeof(pgrc_rsets_timing);
    s->tm.edit = 2;
    s->tm.ms_checks_device = s->ev.ms(0, 1);
    s->tm.ms_desc_device = s->ev.ms(1, 2);
    s->tm.ms_rows_device = s->ev.ms(2, 3);
    s->tm.ms_call = dec_ms_since(t0);
    s->have_timing = true;
    return PGRC_OK;
}

// generateHqReadsIndexesMapping into desc[0] (nh + 1 entries, queued); out: the host copy, or NULL to leave it on the device
static int rs_hq_mapping(pgrc_rsets *s, uint32_t *out) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t A = s->A, nh = A - s->set[1].n - s->set[2].n;
    int e;
    if ((e = s->ev.ensure(s))) return e;
    s->tm = pgrc_rsets_timing{};
    s->have_timing = false;
    HIP_TRY(s, s->ev.record(0, s->stream));
    if ((e = rs_classes(s)) || (e = rs_count(s, RsIsClass{(const uint8_t *)s->cls.p, 0}, A, 0))) return e;
    HIP_TRY(s, s->ev.record(1, s->stream));
    if ((e = pgrc_buf_unpooled(s, s->desc[0], (nh + 1) * 4))) return e;
    uint32_t bad[RS_BAD_WORDS] = {}, tot = 0;
    HIP_TRY(s, hipMemcpyAsync(bad, s->words.p, sizeof bad, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipMemcpyAsync(&tot, (const uint32_t *)s->cnt[0].p + A, 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    if ((e = rs_bad_words(s, bad, "HQ mapping"))) return e;
    if (tot != nh) return rs_fail(s, PGRC_E_PARAM, "HQ mapping: the HQ count is not the reads' count minus the LQ and N counts");
    hipLaunchKernelGGL(k_rs_hq_map, dim3(dec_grid(A + 1, RS_TPB)), dim3(RS_TPB), 0, s->stream, (const uint8_t *)s->cls.p, A, (const uint32_t *)s->cnt[0].p, (uint32_t *)s->desc[0].p);
    HIP_TRY(s, hipGetLastError());
    HIP_TRY(s, s->ev.record(2, s->stream));
    if (out) {
        if ((e = dec_download_host(s, out, s->desc[0].p, (nh + 1) * 4))) return e;
    } else {
        HIP_TRY(s, hipStreamSynchronize(s->stream));
    }
    s->tm.struct_size = sizeof(pgrc_rsets_timing);
    s->tm.edit = 3;
    s->tm.ms_checks_device = s->ev.ms(0, 1);
    s->tm.ms_desc_device = s->ev.ms(1, 2);
    s->tm.ms_call = dec_ms_since(t0);
    s->have_timing = true;
    return PGRC_OK;
}

// one batch: rows and batch-local indexes in host memory (on_device = false) or in memory of this device.  The batch's indexes
// are checked before anything of the object changes: what is written lies behind the sets' counts until the call has succeeded.
static int rs_append(pgrc_rsets *s, const uint64_t cnt[3], const uint8_t *const rows[3], const uint32_t *const idx[2], uint64_t n_records, bool on_device) {
    int e;
    if (!n_records) return PGRC_OK;
    // the indexes on the device, batch-local, behind one another in stage_idx
    const uint64_t ni = cnt[1] + cnt[2];
    if ((e = pgrc_buf_unpooled(s, s->stage_idx, (ni + 1) * 4))) return e;
    uint32_t *loc[2] = {(uint32_t *)s->stage_idx.p, (uint32_t *)s->stage_idx.p + cnt[1]};
    for (int k = 0; k < 2; k++) {
        if (!cnt[k + 1]) continue;
        if (on_device) HIP_TRY(s, hipMemcpyAsync(loc[k], idx[k], cnt[k + 1] * 4, hipMemcpyDeviceToDevice, s->stream));
        else if ((e = dec_upload_host(s, loc[k], idx[k], cnt[k + 1] * 4))) return e;
    }
    if ((e = rs_classes_of(s, n_records, loc[0], cnt[1], loc[1], cnt[2]))) return e;
    uint32_t bad[RS_BAD_WORDS] = {};
    HIP_TRY(s, hipMemcpyAsync(bad, s->words.p, sizeof bad, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    if ((e = rs_bad_words(s, bad, "append"))) return e;
    for (int k = 0; k < 3; k++)
        if ((e = rs_reserve(s, s->set[k], s->set[k].n + cnt[k], k ? s->set[k].n + cnt[k] + 1 : 0))) return e;
    for (int k = 0; k < 3; k++) {
        RsSet &t = s->set[k];
        if (!cnt[k]) continue;
        uint8_t *dst = (uint8_t *)t.rows.p + t.n * t.rb;
        if (on_device) HIP_TRY(s, hipMemcpyAsync(dst, rows[k], cnt[k] * t.rb, hipMemcpyDeviceToDevice, s->stream));
        else if ((e = dec_upload_host(s, dst, rows[k], cnt[k] * t.rb))) return e;
        if (k) hipLaunchKernelGGL(k_rs_offset, dim3(dec_grid(cnt[k], RS_TPB)), dim3(RS_TPB), 0, s->stream, (const uint32_t *)loc[k - 1], cnt[k], (uint32_t)s->A, (uint32_t *)t.map.p + t.n);
    }
    HIP_TRY(s, hipGetLastError());
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    for (int k = 0; k < 3; k++) s->set[k].n += cnt[k];
    s->A += n_records;
    return PGRC_OK;
}

static int rs_append_checks(pgrc_rsets *s, const uint64_t cnt[3], const uint32_t sym[3], const uint32_t rb[3], uint64_t n_records) {
    if (s->finished) return rs_fail(s, PGRC_E_STATE, "append after pgrc_rsets_finish");
    if (n_records > 0xFFFFFFFEull || s->A + n_records > 0xFFFFFFFEull) return rs_fail(s, PGRC_E_PARAM, "append: more than 2^32 - 2 reads");
    if (cnt[0] > n_records || cnt[1] > n_records || cnt[2] > n_records || cnt[0] + cnt[1] + cnt[2] != n_records)
        return rs_fail(s, PGRC_E_PARAM, "append: the HQ count is not the records' count minus the LQ and N counts");
    for (int k = 0; k < 3; k++) {
        if (!s->set[k].symbols && cnt[k]) return rs_fail(s, PGRC_E_PARAM, "append: reads for the N set, which this object does not have");
        if (cnt[k] && (sym[k] != s->set[k].symbols || rb[k] != s->set[k].rb)) return rs_fail(s, PGRC_E_PARAM, "append: the batch's alphabets or row bytes are not this object's");
    }
    return PGRC_OK;
}

extern "C" {

const char *pgrc_rsets_last_error(const pgrc_rsets *s) { return s ? s->err.c_str() : g_rs_create_err.c_str(); }

int pgrc_rsets_create(const pgrc_rsets_params *p, pgrc_rsets **out) {
    if (!out) return PGRC_E_PARAM;
    *out = nullptr;
    if (!p) { g_rs_create_err = "read sets: params is NULL"; return PGRC_E_PARAM; }
    if (p->struct_size != sizeof(pgrc_rsets_params)) { g_rs_create_err = "read sets: struct_size is not sizeof(pgrc_rsets_params)"; return PGRC_E_PARAM; }
    if (p->read_len < 1 || p->read_len > 255) { g_rs_create_err = "read sets: the read length must be in [1, 255]"; return PGRC_E_PARAM; }
    pgrc_rsets *s = new pgrc_rsets();
    std::string why;
    const int e = pgrc_stage_open(s, p->device, &why);
    if (e) {
        g_rs_create_err = "read sets: " + why;
        delete s;
        return e;
    }
    s->prm = *p;
    // the alphabets (DividedPCLReadsSets.cpp:10-21)
    const bool n_apart = p->separate_n_reads_set || p->n_reads_lq;
    const uint32_t sym[3] = {n_apart ? 4u : 5u, p->separate_n_reads_set ? 4u : 5u, p->separate_n_reads_set ? 5u : 0u};
    for (int k = 0; k < 3; k++) {
        s->set[k].symbols = sym[k];
        s->set[k].rb = sym[k] == 4 ? (p->read_len + 3) / 4 : sym[k] == 5 ? (p->read_len + 2) / 3 : 0;
    }
    *out = s;
    return PGRC_OK;
}

void pgrc_rsets_destroy(pgrc_rsets *s) {
    if (!s) return;
    PgrcDeviceScope scope(s->device);
    (void)hipStreamSynchronize(s->stream);
    dec_free_all(rs_bufs(s));
    s->ev.release();
    pgrc_stage_close(s);
    delete s;
}

int pgrc_rsets_append(pgrc_rsets *s, const pgrc_divided_reads *b, uint64_t n_records) {
    if (!s) return PGRC_E_PARAM;
    if (!b) return rs_fail(s, PGRC_E_PARAM, "append: batch is NULL");
    const uint64_t cnt[3] = {b->n_hq, b->n_lq, b->n_n};
    const uint32_t sym[3] = {b->hq_symbols, b->lq_symbols, b->n_symbols}, rb[3] = {b->hq_row_bytes, b->lq_row_bytes, b->n_row_bytes};
    const uint8_t *rows[3] = {b->hq_rows, b->lq_rows, b->n_rows};
    const uint32_t *idx[2] = {b->lq_index, b->n_index};
    int e;
    if ((e = rs_append_checks(s, cnt, sym, rb, n_records))) return e;
    for (int k = 0; k < 3; k++)
        if (cnt[k] && (!rows[k] || (k && !idx[k - 1]))) return rs_fail(s, PGRC_E_PARAM, "append: a set of the batch has reads and a NULL array");
    PGRC_ON_DEVICE(s);
    e = rs_append(s, cnt, rows, idx, n_records, false);
    if (e) (void)hipStreamSynchronize(s->stream);
    return e;
}

int pgrc_rsets_append_divider(pgrc_rsets *s, pgrc_divider *dv) {
    if (!s) return PGRC_E_PARAM;
    if (!dv) return rs_fail(s, PGRC_E_PARAM, "append: divider is NULL");
    PgrcDividerLast l;
    pgrc_divider_last_device(dv, &l);
    if (l.device != s->device) return rs_fail(s, PGRC_E_PARAM, "append: the divider is on another device");
    if (l.prm.read_len != s->prm.read_len || !l.prm.separate_n_reads_set != !s->prm.separate_n_reads_set || !l.prm.n_reads_lq != !s->prm.n_reads_lq)
        return rs_fail(s, PGRC_E_PARAM, "append: the divider's read length or set arguments are not this object's");
    if (s->finished) return rs_fail(s, PGRC_E_STATE, "append after pgrc_rsets_finish");
    if (!l.valid) return rs_fail(s, PGRC_E_STATE, "append: the divider's last run failed, or it has made none");
    int e;
    if ((e = rs_append_checks(s, l.cnt, l.symbols, l.rb, l.n_records))) return e;
    PGRC_ON_DEVICE(s);
    e = rs_append(s, l.cnt, l.d_rows, l.d_idx, l.n_records, true);
    if (e) (void)hipStreamSynchronize(s->stream);
    return e;
}

int pgrc_rsets_finish(pgrc_rsets *s) {
    if (!s) return PGRC_E_PARAM;
    if (s->finished) return rs_fail(s, PGRC_E_STATE, "finish: already finished");
    PGRC_ON_DEVICE(s);
    int e;
    if (s->set[0].n != s->A - s->set[1].n - s->set[2].n) return rs_fail(s, PGRC_E_PARAM, "finish: the HQ count is not the reads' count minus the LQ and N counts");
    for (int k = 1; k < 3; k++) {
        RsSet &t = s->set[k];
        if (!t.symbols) continue;
        if ((e = rs_reserve(s, t, t.n, t.n + 1))) return e;
        const uint32_t guard = (uint32_t)s->A;
        HIP_TRY(s, hipMemcpyAsync((uint32_t *)t.map.p + t.n, &guard, 4, hipMemcpyHostToDevice, s->stream));
        HIP_TRY(s, hipStreamSynchronize(s->stream));
    }
    if ((e = rs_classes(s))) return e;
    uint32_t bad[RS_BAD_WORDS] = {};
    HIP_TRY(s, hipMemcpyAsync(bad, s->words.p, sizeof bad, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    if ((e = rs_bad_words(s, bad, "finish"))) return e;
    s->finished = true;
    return PGRC_OK;
}

int pgrc_rsets_get_info(pgrc_rsets *s, pgrc_rsets_info *out) {
    if (!s) return PGRC_E_PARAM;
    if (!out || out->struct_size != sizeof(pgrc_rsets_info)) return rs_fail(s, PGRC_E_PARAM, "info is NULL or struct_size is not sizeof(pgrc_rsets_info)");
    *out = pgrc_rsets_info{};
    out->struct_size = sizeof(pgrc_rsets_info);
    out->finished = s->finished;
    out->reads_total_count = s->A;
    for (int k = 0; k < 3; k++) {
        out->count[k] = s->set[k].n;
        out->symbols[k] = s->set[k].symbols;
        out->row_bytes[k] = s->set[k].rb;
        out->disposed[k] = s->set[k].disposed;
    }
    return PGRC_OK;
}

static int rs_which(pgrc_rsets *s, int32_t which, const char *what) {
    if (which < 0 || which > 2) return rs_fail(s, PGRC_E_PARAM, std::string(what) + ": which is PGRC_RSETS_HQ, PGRC_RSETS_LQ or PGRC_RSETS_N");
    if (!s->set[which].symbols) return rs_fail(s, PGRC_E_PARAM, std::string(what) + ": this object has no N set");
    return PGRC_OK;
}

int pgrc_rsets_get_rows(pgrc_rsets *s, int32_t which, uint64_t first, uint64_t n, uint8_t *out) {
    if (!s) return PGRC_E_PARAM;
    int e;
    if ((e = rs_which(s, which, "get_rows"))) return e;
    RsSet &t = s->set[which];
    if (t.disposed) return rs_fail(s, PGRC_E_STATE, "get_rows: the set has been disposed");
    if (first > t.n || n > t.n - first) return rs_fail(s, PGRC_E_PARAM, "get_rows: rows outside the set");
    if (!out && n) return rs_fail(s, PGRC_E_PARAM, "get_rows: out is NULL");
    PGRC_ON_DEVICE(s);
    return dec_download_host(s, out, (const uint8_t *)t.rows.p + first * t.rb, n * t.rb);
}

int pgrc_rsets_get_mapping(pgrc_rsets *s, int32_t which, uint32_t *out) {
    if (!s) return PGRC_E_PARAM;
    int e;
    if ((e = rs_which(s, which, "get_mapping"))) return e;
    if (!out) return rs_fail(s, PGRC_E_PARAM, "get_mapping: out is NULL");
    if (which == PGRC_RSETS_HQ) {
        if ((e = rs_need(s, "get_mapping", {1, 2}))) return e;
        PGRC_ON_DEVICE(s);
        e = rs_hq_mapping(s, out);
        if (e) (void)hipStreamSynchronize(s->stream);
        return e;
    }
    if ((e = rs_need(s, "get_mapping", {which}))) return e;
    PGRC_ON_DEVICE(s);
    return dec_download_host(s, out, s->set[which].map.p, (s->set[which].n + 1) * 4);
}

int pgrc_rsets_dispose(pgrc_rsets *s, int32_t which) {
    if (!s) return PGRC_E_PARAM;
    if (which < 0 || which > 2) return rs_fail(s, PGRC_E_PARAM, "dispose: which is PGRC_RSETS_HQ, PGRC_RSETS_LQ or PGRC_RSETS_N");
    RsSet &t = s->set[which];
    PGRC_ON_DEVICE(s);
    (void)hipStreamSynchronize(s->stream);
    dec_free(t.rows);
    dec_free(t.map);
    t.cap_rows = t.cap_map = 0;
    t.disposed = true;
    if (which == PGRC_RSETS_HQ) s->hq_gen++;
    return PGRC_OK;
}

int pgrc_rsets_move_lq(pgrc_rsets *s, const uint8_t *is_hq, int32_t flags_on_device) {
    if (!s) return PGRC_E_PARAM;
    int e;
    if (!is_hq && s->set[0].n) return rs_fail(s, PGRC_E_PARAM, "move: is_hq is NULL");
    if ((e = rs_need(s, "move", {0, 1, 2})) || (e = rs_move_allowed(s))) return e;
    PGRC_ON_DEVICE(s);
    const uint8_t *d_flags = nullptr;
    if ((e = rs_flags(s, is_hq, s->set[0].n, flags_on_device, &d_flags)) || (e = rs_move(s, d_flags))) (void)hipStreamSynchronize(s->stream);
    return e;
}

int pgrc_rsets_move_by_overlap(pgrc_rsets *s, pgrc_ovl_ctx *ovl) {
    if (!s) return PGRC_E_PARAM;
    if (!ovl) return rs_fail(s, PGRC_E_PARAM, "move: the overlap context is NULL");
    int e;
    if ((e = rs_need(s, "move", {0, 1, 2})) || (e = rs_move_allowed(s))) return e;
    if (pgovl_device(ovl) != s->device) return rs_fail(s, PGRC_E_PARAM, "move: the overlap context is on another device");
    if (s->ovl_ctx != ovl || !s->ovl_serial || pgovl_run_serial(ovl) != s->ovl_serial || s->ovl_gen != s->hq_gen)
        return rs_fail(s, PGRC_E_STATE, "move: the overlap context's last run was not made by pgrc_rsets_overlap on this object's HQ set as it is now");
    const uint8_t *d_flags = nullptr;
    uint64_t R = 0;
    if ((e = pgovl_both_sides_device(ovl, &d_flags, &R))) return rs_fail(s, e, std::string("move: ") + pgrc_ovl_last_error(ovl));
    if (R != s->set[0].n) return rs_fail(s, PGRC_E_STATE, "move: the overlap context's run has another reads' count than the HQ set");
    PGRC_ON_DEVICE(s);
    if ((e = rs_move(s, d_flags))) (void)hipStreamSynchronize(s->stream);
    return e;
}

int pgrc_rsets_remove(pgrc_rsets *s, const uint8_t *is_mapped, int32_t flags_on_device) {
    if (!s) return PGRC_E_PARAM;
    int e;
    const uint64_t n = s->set[1].n + s->set[2].n;
    if (!is_mapped && n) return rs_fail(s, PGRC_E_PARAM, "remove: is_mapped is NULL");
    if ((e = rs_need(s, "remove", {1, 2}))) return e;
    PGRC_ON_DEVICE(s);
    const uint8_t *d_flags = nullptr;
    if ((e = rs_flags(s, is_mapped, n, flags_on_device, &d_flags)) || (e = rs_remove(s, d_flags))) (void)hipStreamSynchronize(s->stream);
    return e;
}

int pgrc_rsets_remove_matched(pgrc_rsets *s, pgrc_match_ctx *c) {
    if (!s) return PGRC_E_PARAM;
    if (!c) return rs_fail(s, PGRC_E_PARAM, "remove: the matcher is NULL");
    int e;
    if ((e = rs_need(s, "remove", {1, 2}))) return e;
    const uint64_t n = s->set[1].n + s->set[2].n;
    if (c->multi) return rs_fail(s, PGRC_E_PARAM, "remove: the matcher runs on several devices");
    if (c->device != s->device) return rs_fail(s, PGRC_E_PARAM, "remove: the matcher is on another device");
    if (!c->rd.have_reads || c->rd.n != n) return rs_fail(s, PGRC_E_PARAM, "remove: the matcher's read count is not the LQ count plus the N count");
    if (!c->res.have_results || !c->res.d_pos.p) return rs_fail(s, PGRC_E_STATE, "remove: the matcher has no results");
    PGRC_ON_DEVICE(s);
    HIP_TRY(s, hipStreamSynchronize(c->stream));
    if ((e = pgrc_buf_unpooled(s, s->flags, n + 16))) return e;
    if (n) hipLaunchKernelGGL(k_rs_matched, dim3(dec_grid(n, RS_TPB)), dim3(RS_TPB), 0, s->stream, (const uint64_t *)c->res.d_pos.p, n, (uint8_t *)s->flags.p);
    HIP_TRY(s, hipGetLastError());
    if ((e = rs_remove(s, (const uint8_t *)s->flags.p))) (void)hipStreamSynchronize(s->stream);
    return e;
}

int pgrc_rsets_overlap(pgrc_rsets *s, int32_t which, pgrc_ovl_ctx *ovl, double stop_coef, uint32_t overlap_width, const uint32_t *sorted_order, pgrc_ovl_result *out) {
    if (!s) return PGRC_E_PARAM;
    if (out) *out = pgrc_ovl_result{};
    if (!ovl || !out) return rs_fail(s, PGRC_E_PARAM, "overlap: the overlap context or out is NULL");
    int e;
    if ((e = rs_which(s, which, "overlap")) || (e = rs_need(s, "overlap", {which}))) return e;
    if (pgovl_device(ovl) != s->device) return rs_fail(s, PGRC_E_PARAM, "overlap: the overlap context is on another device");
    const RsSet &t = s->set[which];
    if (!t.n) return rs_fail(s, PGRC_E_PARAM, "overlap: the set is empty");
    pgrc_ovl_input in{};
    in.struct_size = sizeof(in);
    in.read_len = s->prm.read_len;
    in.symbols = t.symbols;
    in.overlap_width = overlap_width;
    in.n_reads = t.n;
    in.stop_coef = stop_coef;
    in.packed_rows = (const uint8_t *)t.rows.p;
    in.sorted_order = sorted_order;
    if (s->ovl_ctx == ovl) s->ovl_ctx = nullptr;
    if ((e = pgovl_run_rows(ovl, &in, out, true))) return rs_fail(s, e, std::string("overlap: ") + pgrc_ovl_last_error(ovl));
    if (which == PGRC_RSETS_HQ) {
        s->ovl_ctx = ovl;
        s->ovl_serial = pgovl_run_serial(ovl);
        s->ovl_gen = s->hq_gen;
    }
    return PGRC_OK;
}

int pgrc_rsets_to_matcher(pgrc_rsets *s, pgrc_match_ctx *c) {
    if (!s) return PGRC_E_PARAM;
    if (!c) return rs_fail(s, PGRC_E_PARAM, "to_matcher: the matcher is NULL");
    int e;
    if ((e = rs_need(s, "to_matcher", {1, 2}))) return e;
    if (c->multi) return rs_fail(s, PGRC_E_PARAM, "to_matcher: the matcher runs on several devices");
    if (pgrc_stream_active(c)) return rs_fail(s, PGRC_E_PARAM, "to_matcher: the matcher is in a streamed run");
    if (c->device != s->device) return rs_fail(s, PGRC_E_PARAM, "to_matcher: the matcher is on another device");
    if (c->prm.read_len != s->prm.read_len) return rs_fail(s, PGRC_E_PARAM, "to_matcher: the matcher has another read length");
    const RsSet &lq = s->set[1], &nn = s->set[2];
    e = pgrc_match_begin_reads(c, lq.n + nn.n);
    if (!e && lq.n) e = pgrc_append_rows_device(c, (const uint8_t *)lq.rows.p, lq.n, (int32_t)lq.symbols);
    if (!e && nn.n) e = pgrc_append_rows_device(c, (const uint8_t *)nn.rows.p, nn.n, (int32_t)nn.symbols);
    if (!e) e = pgrc_match_end_reads(c);
    if (e) {
        const std::string why = pgrc_match_last_error(c);
        pgrc_upload_close(c);       // the sequence that begin_reads opened does not stay open: the matcher has no reads until its next begin
        return rs_fail(s, e, "to_matcher: " + why);
    }
    return PGRC_OK;
}

int pgrc_rsets_get_timing(pgrc_rsets *s, pgrc_rsets_timing *out) {
    if (!s) return PGRC_E_PARAM;
    if (!out || out->struct_size != sizeof(pgrc_rsets_timing)) return rs_fail(s, PGRC_E_PARAM, "timing is NULL or struct_size is not sizeof(pgrc_rsets_timing)");
    if (!s->have_timing) return rs_fail(s, PGRC_E_STATE, "no edit has succeeded on this object");
    *out = s->tm;
    return PGRC_OK;
}

}   // extern "C"

// rlistctx.h: the mapping of set `which` where it lies on the device, *entries indexes in front of the guard.  HQ: made by the
// code of pgrc_rsets_get_mapping into scratch of the object, valid until its next edit or get_mapping
int pgrc_rsets_mapping_device(pgrc_rsets *s, int32_t which, const uint32_t **d_map, uint64_t *entries) {
    int e;
    if ((e = rs_which(s, which, "mapping"))) return e;
    if (which == PGRC_RSETS_HQ) {
        if ((e = rs_need(s, "mapping", {1, 2}))) return e;
        PGRC_ON_DEVICE(s);
        if ((e = rs_hq_mapping(s, nullptr))) {
            (void)hipStreamSynchronize(s->stream);
            return e;
        }
        *d_map = (const uint32_t *)s->desc[0].p;
        *entries = s->A - s->set[1].n - s->set[2].n;
        return PGRC_OK;
    }
    if ((e = rs_need(s, "mapping", {which}))) return e;
    *d_map = (const uint32_t *)s->set[which].map.p;
    *entries = s->set[which].n;
    return PGRC_OK;
}
