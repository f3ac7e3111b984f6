// rlist.hip -- a pseudogenome's reads list on the device from the assembly to the archive (include/pgrc_readslist.h,
// DESIGN.md 4.20): off (16 bits), orgIdx, revComp and the mismatch streams of the list the second half of the encoder works on
// (pgrc/pgrc-encoder.cpp: runHQPgGeneration .. compressReadsOrder), with the stages that fill it and the ones that consume it.
//
// Most of the work is done by the kernels of the stages themselves behind device-source switches (rlistctx.h): export.hip's
// merge, listarchive.hip's reshaping, pairorder.hip's and pairpos.hip's coders.  What is new here:
//   the mapping gather      applyIndexesMapping, org[j] = map[org[j]], the mapping read where pgrc_rsets keeps it
//   the narrowing of off    16 -> 8 bits on the way into the archive block (8 offsets per thread: one 16-byte load, one 8-byte store)
//   the joined feed         the three lists' orgIdx one behind the other, as compressReadsOrder numbers the entries
//   the position array      orgIdx2PgPos: the shared scan of off whose output functor scatters base + sum at org[i] and marks the
//                           index's class byte; a second pass reads every write back; one pass over the T class bytes finds an
//                           index nobody wrote.  With the writers' count equal to T that proves "every index exactly once"
//                           without a sort and without an atomic
//   the narrowing of it     64 -> 32 bits for the single-file order-preserving mode, which writes the array itself
// The order-preserving mode's export (export.hip's entry list behind a second resident door) goes into a list of its own, and
// its archive block starts at revComp: that mode writes neither off nor orgIdx.
// Producers build the new content beside the old one and swap it in on success.  No library kernel.
#include <stdlib.h>

#include <chrono>

#include "devutil.h"
#include "pgrc_readslist_ord.h"
#include "rlistctx.h"

#define RL_TPB 256
#define RL_MAX_BLOCKS (1u << 18)

// the words of `words`
enum { RL_BAD_RANGE, RL_BAD_TWICE, RL_BAD_NEVER, RL_BAD_WIDE, RL_BAD_WORDS };

static thread_local std::string g_rl_create_err;

static inline uint32_t rl_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + RL_TPB - 1) / RL_TPB, 1), RL_MAX_BLOCKS); }
static int rl_fail(pgrc_rlist *s, int code, const std::string &msg) { return dec_fail(s, code, "reads list: " + msg); }

// ------------------------------------------------------------------------------------------------ kernels
// applyIndexesMapping; an index at or above the mapping's count sets bad[RL_BAD_RANGE] and reads nothing
static __global__ void __launch_bounds__(RL_TPB) k_rl_map(const uint32_t *__restrict__ org, uint64_t n, const uint32_t *__restrict__ map, uint64_t count,
                                                          uint32_t *__restrict__ out, uint32_t *__restrict__ bad) {
    for (uint64_t j = (uint64_t)blockIdx.x * RL_TPB + threadIdx.x; j < n; j += (uint64_t)gridDim.x * RL_TPB) {
        const uint32_t v = org[j];
        if (v >= count) bad[RL_BAD_RANGE] = 1;
        else out[j] = map[v];
    }
}

// off in one byte each (writeReadLengthValue with bytePerReadLengthMode stores the low byte); in and out are 16-byte aligned
static __global__ void __launch_bounds__(RL_TPB) k_rl_narrow(const uint16_t *__restrict__ in, uint64_t n, uint8_t *__restrict__ out) {
    const uint64_t groups = n >> 3;
    for (uint64_t g = (uint64_t)blockIdx.x * RL_TPB + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * RL_TPB) {
        const uint4 v = reinterpret_cast<const uint4 *>(in)[g];
        uint2 o;
        o.x = (v.x & 0xFFu) | ((v.x >> 8) & 0xFF00u) | ((v.y & 0xFFu) << 16) | ((v.y << 8) & 0xFF000000u);
        o.y = (v.z & 0xFFu) | ((v.z >> 8) & 0xFF00u) | ((v.w & 0xFFu) << 16) | ((v.w << 8) & 0xFF000000u);
        reinterpret_cast<uint2 *>(out)[g] = o;
    }
    const uint64_t t = (groups << 3) + (uint64_t)blockIdx.x * RL_TPB + threadIdx.x;     // the last n % 8 offsets
    if (t < n) out[t] = (uint8_t)in[t];
}

static __global__ void __launch_bounds__(RL_TPB) k_rl_widen(const uint8_t *__restrict__ in, uint64_t n, uint16_t *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * RL_TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RL_TPB) out[i] = in[i];
}

// the entries of HQ | LQ | N as compressReadsOrder numbers them (end[l]: the entries up to and including list l)
struct RlJoin {
    const uint32_t *p[3];
    uint64_t end[3];
};
static __global__ void __launch_bounds__(RL_TPB) k_rl_join(const RlJoin a, uint32_t *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * RL_TPB + threadIdx.x; i < a.end[2]; i += (uint64_t)gridDim.x * RL_TPB)
        out[i] = i < a.end[0] ? a.p[0][i] : i < a.end[1] ? a.p[1][i - a.end[0]] : a.p[2][i - a.end[1]];
}

// one write of the position array, or (check) its read-back: a second writer of an index has replaced the value or the class
__device__ __forceinline__ void rl_pos_put(uint64_t idx, uint64_t v, uint8_t c, bool check, uint64_t T, uint64_t *__restrict__ pos, uint8_t *__restrict__ cls,
                                           uint32_t *__restrict__ bad) {
    if (idx >= T) {
        bad[RL_BAD_RANGE] = 1;
    } else if (!check) {
        pos[idx] = v;
        cls[idx] = c;
    } else if (pos[idx] != v || cls[idx] != c) {
        bad[RL_BAD_TWICE] = 1;
    }
}

// the output functor of the scan over a list's off: entry i lies at v = base + off[0] + .. + off[i]
struct RlPosOut {
    const uint32_t *org;
    uint64_t T;
    uint64_t *pos;
    uint8_t *cls;
    uint32_t *bad;
    uint8_t c;
    bool check;
    __device__ void operator()(uint64_t i, uint64_t v) const { rl_pos_put(org[i], v, c, check, T, pos, cls, bad); }
};

// the matcher's matched reads (ReadsMatchers.cpp:659); rorg: the reads' original indexes, NULL = identity
static __global__ void __launch_bounds__(RL_TPB) k_rl_pos_matched(const uint64_t *__restrict__ mpos, uint64_t n, const uint32_t *__restrict__ rorg, uint64_t T, bool check,
                                                                  uint64_t *__restrict__ pos, uint8_t *__restrict__ cls, uint32_t *__restrict__ bad) {
    for (uint64_t r = (uint64_t)blockIdx.x * RL_TPB + threadIdx.x; r < n; r += (uint64_t)gridDim.x * RL_TPB) {
        const uint64_t p = mpos[r];
        if (p != PGRC_NOT_MATCHED_POS) rl_pos_put(rorg ? rorg[r] : r, p, 4, check, T, pos, cls, bad);
    }
}

static __global__ void __launch_bounds__(RL_TPB) k_rl_pos_never(const uint8_t *__restrict__ cls, uint64_t T, uint32_t *__restrict__ bad) {
    for (uint64_t t = (uint64_t)blockIdx.x * RL_TPB + threadIdx.x; t < T; t += (uint64_t)gridDim.x * RL_TPB)
        if (!cls[t]) bad[RL_BAD_NEVER] = 1;
}

// orgIdx2PgPos in four bytes each (compressReadsPgPositions' singleFileMode, SeparatedPseudoGenomePersistence.cpp:454-459); a
// position that does not fit sets bad[RL_BAD_WIDE]
static __global__ void __launch_bounds__(RL_TPB) k_rl_pos_narrow(const uint64_t *__restrict__ pos, uint64_t T, uint32_t *__restrict__ out, uint32_t *__restrict__ bad) {
    for (uint64_t t = (uint64_t)blockIdx.x * RL_TPB + threadIdx.x; t < T; t += (uint64_t)gridDim.x * RL_TPB) {
        const uint64_t p = pos[t];
        if (p >> 32) bad[RL_BAD_WIDE] = 1;
        out[t] = (uint32_t)p;
    }
}

// ------------------------------------------------------------------------------------------------ host side: helpers
static DevBufList rl_bufs(pgrc_rlist *s) { return {&s->map, &s->words, &s->block, &s->join, &s->pos, &s->scan, &s->cls}; }

static void rl_free(RlBufs &b) {
    dec_free_all({&b.off, &b.org, &b.rc, &b.cnt, &b.sym, &b.roff});
    b = RlBufs{};
}

// fresh buffers of exactly the list's sizes; given back by the caller if its call fails
static int rl_alloc(PgrcStage *s, RlBufs &b, uint64_t n, uint64_t m, bool rc, bool mis, uint32_t off_width) {
    int e;
    if ((e = pgrc_bufs_unpooled(s, {{&b.off, n * 2 + 16}, {&b.org, n * 4 + 16}}))) return e;
    if (rc && (e = pgrc_buf_unpooled(s, b.rc, n + 16))) return e;
    if (mis && (e = pgrc_bufs_unpooled(s, {{&b.cnt, n + 16}, {&b.sym, m + 16}, {&b.roff, m * off_width + 16}}))) return e;
    b.n = n;
    b.nmis = m;
    b.has_rc = rc;
    b.has_mis = mis;
    b.off_width = off_width;
    return PGRC_OK;
}

static void rl_swap_in(pgrc_rlist *s, RlBufs &nb) {
    rl_free(s->cur);
    s->cur = nb;
    nb = RlBufs{};
}

static int rl_events(pgrc_rlist *s) {
    if (int e = s->ev.ensure(s)) return e;
    for (hipEvent_t &ev : s->ev_x)
        if (!ev) HIP_TRY(s, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return PGRC_OK;
}

static int rl_begin(pgrc_rlist *s) {
    int e;
    if ((e = rl_events(s))) return e;
    s->have_timing = false;
    s->tm = pgrc_rlist_timing{};
    HIP_TRY(s, s->ev.record(0, s->stream));
    return PGRC_OK;
}

// the stream is idle: ev[0 .. 3] have been recorded in order
static void rl_done(pgrc_rlist *s, uint32_t call, std::chrono::steady_clock::time_point t0) {
    s->tm.struct_size = sizeof(pgrc_rlist_timing);
    s->tm.call = call;
    s->tm.ms_fetch_device = s->ev.ms(0, 1);
    s->tm.ms_build_device = s->ev.ms(1, 2);
    s->tm.ms_pack_device = s->ev.ms(2, 3);
    s->tm.ms_call = dec_ms_since(t0);
    s->have_timing = true;
}

static int rl_copy(pgrc_rlist *s, void *dst, const void *src, uint64_t bytes) {
    if (!bytes) return PGRC_OK;
    HIP_TRY(s, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s->stream));
    s->tm.bytes_device_copy += bytes;
    return PGRC_OK;
}

static int rl_narrow(pgrc_rlist *s, const uint16_t *in, uint64_t n, uint8_t *out) {
    if (!n) return PGRC_OK;
    hipLaunchKernelGGL(k_rl_narrow, dim3(rl_grid(std::max<uint64_t>(n >> 3, 8))), dim3(RL_TPB), 0, s->stream, in, n, out);
    HIP_TRY(s, hipGetLastError());
    return PGRC_OK;
}

// the original indexes of a matcher's reads from the read sets: SumOfMappings of the LQ and the N mapping, joined in `map`
static int rl_reads_org(pgrc_rlist *s, pgrc_rsets *sets, uint64_t matcher_n, const char *what, const uint32_t **d_rorg) {
    if (sets->device != s->device) return rl_fail(s, PGRC_E_PARAM, std::string(what) + ": the read sets are on another device");
    const uint32_t *m[2] = {};
    uint64_t cnt[2] = {};
    int e;
    for (int k = 1; k <= 2; k++) {
        if (!sets->set[k].symbols) continue;
        if ((e = pgrc_rsets_mapping_device(sets, k, &m[k - 1], &cnt[k - 1]))) return rl_fail(s, e, std::string(what) + ": " + pgrc_rsets_last_error(sets));
    }
    if (cnt[0] + cnt[1] != matcher_n) return rl_fail(s, PGRC_E_PARAM, std::string(what) + ": the LQ count plus the N count of the read sets is not the matcher's read count");
    if ((e = pgrc_buf_unpooled(s, s->map, matcher_n * 4 + 16))) return e;
    uint32_t *dst = (uint32_t *)s->map.p;
    if ((e = rl_copy(s, dst, m[0], cnt[0] * 4)) || (e = rl_copy(s, dst + cnt[0], m[1], cnt[1] * 4))) return e;
    *d_rorg = dst;
    return PGRC_OK;
}

static int rl_matcher_ok(pgrc_rlist *s, pgrc_match_ctx *c, const char *what) {
    if (c->multi) return rl_fail(s, PGRC_E_PARAM, std::string(what) + ": the matcher runs on several devices");
    if (c->device != s->device) return rl_fail(s, PGRC_E_PARAM, std::string(what) + ": the matcher is on another device");
    return PGRC_OK;
}

// ------------------------------------------------------------------------------------------------ host side: the calls
static int rl_set_host(pgrc_rlist *s, const pgrc_export_streams *in) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n = in->n_entries, m = in->n_mismatches;
    const bool mis = in->mis_cnt != nullptr;
    const uint32_t w = in->off_width;
    int e;
    if ((e = rl_begin(s))) return e;
    RlBufs nb;
    auto run = [&]() -> int {
        if ((e = rl_alloc(s, nb, n, m, in->rev_comp != nullptr, mis, w))) return e;
        if (w == 2) {
            if ((e = dec_upload_host(s, nb.off.p, in->off, n * 2))) return e;
        } else {
            if ((e = pgrc_buf_unpooled(s, s->block, n + 16)) || (e = dec_upload_host(s, s->block.p, in->off, n))) return e;
            if (n) hipLaunchKernelGGL(k_rl_widen, dim3(rl_grid(n)), dim3(RL_TPB), 0, s->stream, (const uint8_t *)s->block.p, n, (uint16_t *)nb.off.p);
            HIP_TRY(s, hipGetLastError());
        }
        if ((e = dec_upload_host(s, nb.org.p, in->org_idx, n * 4))) return e;
        if (nb.has_rc && (e = dec_upload_host(s, nb.rc.p, in->rev_comp, n))) return e;
        s->tm.bytes_up = n * w + n * 4 + (nb.has_rc ? n : 0);
        HIP_TRY(s, s->ev.record(1, s->stream));
        if (mis) {
            if ((e = dec_upload_host(s, nb.cnt.p, in->mis_cnt, n)) || (e = dec_upload_host(s, nb.sym.p, in->mis_sym, m)) || (e = dec_upload_host(s, nb.roff.p, in->mis_rev_off, m * w)))
                return e;
            s->tm.bytes_up += n + m + m * w;
            // the counts describe the streams
            if ((e = pgrc_buf_unpooled(s, s->scan, (n + 1) * 8)) || (e = dec_scan<false>(s, XfU8{(const uint8_t *)nb.cnt.p}, n, 0, (uint64_t *)s->scan.p))) return e;
            uint64_t m_dev = 0;
            HIP_TRY(s, hipMemcpyAsync(&m_dev, (const uint64_t *)s->scan.p + n, 8, hipMemcpyDeviceToHost, s->stream));
            HIP_TRY(s, hipStreamSynchronize(s->stream));
            if (m_dev != m) return rl_fail(s, PGRC_E_PARAM, "set_host: n_mismatches is " + std::to_string(m) + ", the counts sum to " + std::to_string(m_dev));
        }
        HIP_TRY(s, s->ev.record(2, s->stream));
        HIP_TRY(s, s->ev.record(3, s->stream));
        HIP_TRY(s, hipStreamSynchronize(s->stream));
        return PGRC_OK;
    };
    if ((e = run())) {
        (void)hipStreamSynchronize(s->stream);
        rl_free(nb);
        return e;
    }
    nb.last_pos = in->last_pos;
    rl_swap_in(s, nb);
    rl_done(s, PGRC_RLIST_SET_HOST, t0);
    return PGRC_OK;
}

static int rl_from_assembly(pgrc_rlist *s, const PgasmLastList &l, const uint32_t *d_map, uint64_t map_count) {
    const auto t0 = std::chrono::steady_clock::now();
    int e;
    if ((e = rl_begin(s))) return e;
    RlBufs nb;
    auto run = [&]() -> int {
        if ((e = rl_alloc(s, nb, l.n, 0, false, false, 1)) || (e = pgrc_buf_unpooled(s, s->words, 64))) return e;
        uint32_t *bad = (uint32_t *)s->words.p;
        HIP_TRY(s, hipMemsetAsync(bad, 0, 64, s->stream));
        if ((e = rl_copy(s, nb.off.p, l.d_off, l.n * 2))) return e;
        if (d_map) {
            hipLaunchKernelGGL(k_rl_map, dim3(rl_grid(l.n)), dim3(RL_TPB), 0, s->stream, l.d_org, l.n, d_map, map_count, (uint32_t *)nb.org.p, bad);
            HIP_TRY(s, hipGetLastError());
        } else if ((e = rl_copy(s, nb.org.p, l.d_org, l.n * 4))) {
            return e;
        }
        for (int k = 1; k < 4; k++) HIP_TRY(s, s->ev.record(k, s->stream));
        uint32_t h_bad[RL_BAD_WORDS] = {};
        HIP_TRY(s, hipMemcpyAsync(h_bad, bad, sizeof h_bad, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(s, hipStreamSynchronize(s->stream));
        if (h_bad[RL_BAD_RANGE]) return rl_fail(s, PGRC_E_PARAM, "from_assembly: an index at or above the mapping's count " + std::to_string(map_count));
        return PGRC_OK;
    };
    if ((e = run())) {
        (void)hipStreamSynchronize(s->stream);
        rl_free(nb);
        return e;
    }
    nb.last_pos = l.pg_len - l.read_len;
    rl_swap_in(s, nb);
    rl_done(s, PGRC_RLIST_FROM_ASSEMBLY, t0);
    return PGRC_OK;
}

// the list an export of the matcher left in r, copied into fresh buffers and swapped in; r is released either way
static int rl_take_export(pgrc_rlist *s, pgrc_match_ctx *c, PgrcExportResident &r, const char *what, uint32_t call, uint64_t bytes_up,
                          std::chrono::steady_clock::time_point t0) {
    int e;
    RlBufs nb;
    auto run = [&]() -> int {
        HIP_TRY(s, hipEventRecord(s->ev_x[1], c->stream));
        HIP_TRY(s, hipStreamWaitEvent(s->stream, s->ev_x[1], 0));
        HIP_TRY(s, s->ev.record(2, s->stream));
        if (r.n_entries >= (1ull << 32) || r.n_mismatches >= (1ull << 32)) return rl_fail(s, PGRC_E_PARAM, std::string(what) + ": 2^32 entries or mismatches or more");
        const uint64_t n = r.n_entries, m = r.n_mismatches;
        if ((e = rl_alloc(s, nb, n, m, true, true, r.mis_off_width))) return e;
        if ((e = rl_copy(s, nb.off.p, r.d_off, n * 2)) || (e = rl_copy(s, nb.org.p, r.d_org, n * 4)) || (e = rl_copy(s, nb.rc.p, r.d_rc, n)) || (e = rl_copy(s, nb.cnt.p, r.d_cnt, n)) ||
            (e = rl_copy(s, nb.sym.p, r.d_sym, m)) || (e = rl_copy(s, nb.roff.p, r.d_rev_off, m * r.mis_off_width)))
            return e;
        HIP_TRY(s, s->ev.record(3, s->stream));
        HIP_TRY(s, hipStreamSynchronize(s->stream));
        return PGRC_OK;
    };
    e = run();
    if (e) (void)hipStreamSynchronize(s->stream);
    const uint64_t last = r.last_pos;
    pgrc_export_resident_release(&r);
    if (e) {
        rl_free(nb);
        return e;
    }
    nb.last_pos = last;
    rl_swap_in(s, nb);
    s->tm.bytes_up = bytes_up;
    rl_done(s, call, t0);
    // (the export ran on the matcher's stream between ev[1] and ev[2] of this one, which waited for it)
    return PGRC_OK;
}

static int rl_export(pgrc_rlist *s, pgrc_match_ctx *c, const pgrc_rlist_export_args *x) {
    const auto t0 = std::chrono::steady_clock::now();
    int e;
    if ((e = rl_begin(s))) return e;
    PgrcExportListSrc src{};
    src.count = s->cur.n;
    src.d_off = (const uint16_t *)s->cur.off.p;
    src.d_org = (const uint32_t *)s->cur.org.p;
    src.d_rc = s->cur.has_rc ? (const uint8_t *)s->cur.rc.p : nullptr;
    if (x->sets && (e = rl_reads_org(s, x->sets, c->rd.n, "export_pg_order", &src.d_read_org))) return e;
    pgrc_export_pg_order_args a{};
    a.order = x->order;
    a.n_matched = x->n_matched;
    a.read_org_idx = x->read_org_idx;
    a.rev_compl_pair_file = x->rev_compl_pair_file;
    a.byte_per_read_length = x->byte_per_read_length;
    a.order_on_device = x->order_on_device;
    // the matcher's stream waits for what this one has queued, and this one for the export: no device-wide wait
    HIP_TRY(s, s->ev.record(1, s->stream));
    HIP_TRY(s, hipEventRecord(s->ev_x[0], s->stream));
    HIP_TRY(s, hipStreamWaitEvent(c->stream, s->ev_x[0], 0));
    PgrcExportResident r;
    if ((e = pgrc_export_pg_order_resident(c, &a, &src, &r))) return rl_fail(s, e, std::string("export_pg_order: ") + pgrc_match_last_error(c));
    return rl_take_export(s, c, r, "export_pg_order", PGRC_RLIST_EXPORT, (x->order_on_device ? 0 : x->n_matched * 4) + (x->read_org_idx ? c->rd.n * 4 : 0), t0);
}

// exportMatchesInOriginalOrder: nothing of the old list is read; the same two hand-overs between the streams
static int rl_export_org(pgrc_rlist *s, pgrc_match_ctx *c, const pgrc_rlist_export_org_args *x) {
    const auto t0 = std::chrono::steady_clock::now();
    int e;
    if ((e = rl_begin(s))) return e;
    const uint32_t *d_rorg = nullptr;
    if (x->sets && (e = rl_reads_org(s, x->sets, c->rd.n, "export_original_order", &d_rorg))) return e;
    pgrc_export_original_order_args a{};
    a.read_org_idx = x->read_org_idx;
    a.reads_total_count = x->reads_total_count;
    a.pair_file_mode = x->pair_file_mode;
    a.rev_compl_pair_file = x->rev_compl_pair_file;
    a.byte_per_read_length = x->byte_per_read_length;
    HIP_TRY(s, s->ev.record(1, s->stream));
    HIP_TRY(s, hipEventRecord(s->ev_x[0], s->stream));
    HIP_TRY(s, hipStreamWaitEvent(c->stream, s->ev_x[0], 0));
    PgrcExportResident r;
    if ((e = pgrc_export_original_order_resident(c, &a, d_rorg, &r))) return rl_fail(s, e, std::string("export_original_order: ") + pgrc_match_last_error(c));
    return rl_take_export(s, c, r, "export_original_order", PGRC_RLIST_EXPORT_ORIGINAL, x->read_org_idx ? c->rd.n * 4 : 0, t0);
}

static int rl_download_run(pgrc_rlist *s, pgrc_export_streams *out) {
    const auto t0 = std::chrono::steady_clock::now();
    const RlBufs &b = s->cur;
    const uint64_t n = b.n, m = b.nmis, w = b.off_width;
    int e;
    if ((e = rl_begin(s))) return e;
    for (int k = 1; k < 3; k++) HIP_TRY(s, s->ev.record(k, s->stream));
    out->n_entries = n;
    out->n_mismatches = m;
    out->off_width = (uint32_t)w;
    out->last_pos = b.last_pos;
    out->off = (uint8_t *)malloc(std::max<uint64_t>(n * w, 1));
    out->org_idx = (uint32_t *)malloc(std::max<uint64_t>(n * 4, 1));
    out->rev_comp = (uint8_t *)calloc(std::max<uint64_t>(n, 1), 1);
    out->mis_cnt = (uint8_t *)calloc(std::max<uint64_t>(n, 1), 1);
    out->mis_sym = (uint8_t *)malloc(std::max<uint64_t>(m, 1));
    out->mis_rev_off = (uint8_t *)malloc(std::max<uint64_t>(m * w, 1));
    if (!out->off || !out->org_idx || !out->rev_comp || !out->mis_cnt || !out->mis_sym || !out->mis_rev_off) return rl_fail(s, PGRC_E_ALLOC, "download: host allocation failed");
    const void *d_off = b.off.p;
    if (w == 1) {
        if ((e = pgrc_buf_unpooled(s, s->block, dec_a16(n) + 16)) || (e = rl_narrow(s, (const uint16_t *)b.off.p, n, (uint8_t *)s->block.p))) return e;
        d_off = s->block.p;
    }
    HIP_TRY(s, s->ev.record(3, s->stream));
    if ((e = dec_download_host(s, out->off, d_off, n * w)) || (e = dec_download_host(s, out->org_idx, b.org.p, n * 4))) return e;
    if (b.has_rc && (e = dec_download_host(s, out->rev_comp, b.rc.p, n))) return e;
    if (b.has_mis && ((e = dec_download_host(s, out->mis_cnt, b.cnt.p, n)) || (e = dec_download_host(s, out->mis_sym, b.sym.p, m)) || (e = dec_download_host(s, out->mis_rev_off, b.roff.p, m * w)))) return e;
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    s->tm.bytes_down = n * w + n * 4 + (b.has_rc ? n : 0) + (b.has_mis ? n + m + m * w : 0);
    rl_done(s, PGRC_RLIST_DOWNLOAD, t0);
    return PGRC_OK;
}

// ord (pgrc_rlist_archive_encode_ord; the list has RC flags and mismatch streams): the block starts with revComp, no off
static int rl_archive(pgrc_rlist *s, bool fast, bool want_org, bool ord, pgrc_rlist_archive *out) {
    const char *who = ord ? "reads list: archive_encode_ord" : "reads list: archive_encode";
    const auto t0 = std::chrono::steady_clock::now();
    const RlBufs &b = s->cur;
    const uint64_t n = b.n, m = b.nmis, w = b.off_width;
    int e;
    if ((e = rl_begin(s))) return e;
    // the block: off | revComp | orgIdx | the archive form, each 16-byte aligned
    const uint64_t at_rc = ord ? 0 : dec_a16(n * w) + 16, at_org = at_rc + (b.has_rc ? dec_a16(n) + 16 : 0), at_la = at_org + (want_org ? dec_a16(n * 4) + 16 : 0);
    const uint64_t dev_bytes = at_la + (b.has_mis ? pgrc_la_device_bytes(n, m) : 0), host_bytes = at_la + (b.has_mis ? pgrc_la_host_bytes(n, m) : 0) + 16;
    if ((e = pgrc_buf_unpooled(s, s->block, dev_bytes + 16))) return e;
    uint8_t *ob = (uint8_t *)s->block.p;
    HIP_TRY(s, s->ev.record(1, s->stream));
    PgrcLaResident la{};
    if (b.has_mis && (e = pgrc_la_encode_resident(s, s->la, (const uint8_t *)b.cnt.p, (const uint8_t *)b.sym.p, (const uint8_t *)b.roff.p, n, m, fast, ob + at_la, &la))) return e;
    HIP_TRY(s, s->ev.record(2, s->stream));
    if (!ord && (e = w == 1 ? rl_narrow(s, (const uint16_t *)b.off.p, n, ob) : rl_copy(s, ob, b.off.p, n * 2))) return e;
    if (b.has_rc && (e = rl_copy(s, ob + at_rc, b.rc.p, n))) return e;
    if (want_org && (e = rl_copy(s, ob + at_org, b.org.p, n * 4))) return e;
    HIP_TRY(s, s->ev.record(3, s->stream));
    // the streams end where the last of them ends
    const uint64_t end = b.has_mis ? at_la + la.down : want_org ? at_org + n * 4 : b.has_rc ? at_rc + n : n * w;
    const DecBlockLayout<1> h = {{0}, {end}, host_bytes};     // (one part; the props go behind it)
    const void *src[1] = {ob};
    uint8_t *blk = nullptr;
    uint64_t down = 0;
    if ((e = dec_download_block(s, who, h, src, &blk, &down))) return e;
    out->struct_size = sizeof(pgrc_rlist_archive);
    out->off_width = (uint32_t)w;
    out->n_entries = n;
    out->off = ord ? nullptr : blk;
    out->rev_comp = b.has_rc ? blk + at_rc : nullptr;
    out->org_idx = want_org ? (const uint32_t *)(blk + at_org) : nullptr;
    out->block_bytes = down;
    out->block = blk;
    if (b.has_mis) pgrc_la_describe_resident(&out->archive, blk + at_la, n, m, fast, &la);
    s->tm.bytes_down = down;
    rl_done(s, PGRC_RLIST_ARCHIVE, t0);
    return PGRC_OK;
}

static int rl_pair_order(pgrc_rlist *s, pgrc_rlist *const lists[3], uint64_t T, int32_t form, pgrc_pairorder_streams *out) {
    const auto t0 = std::chrono::steady_clock::now();
    int e;
    if ((e = rl_begin(s))) return e;
    if ((e = pgrc_buf_unpooled(s, s->join, T * 4 + 16))) return e;
    RlJoin j{};
    uint64_t end = 0;
    for (int l = 0; l < 3; l++) {
        j.p[l] = lists[l] ? (const uint32_t *)lists[l]->cur.org.p : nullptr;
        end += lists[l] ? lists[l]->cur.n : 0;
        j.end[l] = end;
    }
    if (T) hipLaunchKernelGGL(k_rl_join, dim3(rl_grid(T)), dim3(RL_TPB), 0, s->stream, j, (uint32_t *)s->join.p);
    HIP_TRY(s, hipGetLastError());
    HIP_TRY(s, s->ev.record(1, s->stream));
    if ((e = pgrc_pairorder_encode_joined(s, s->po, (const uint32_t *)s->join.p, T, form, out))) return e;
    for (int k = 2; k < 4; k++) HIP_TRY(s, s->ev.record(k, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    s->tm.bytes_down = s->po.tm.bytes_down;
    rl_done(s, PGRC_RLIST_PAIR_ORDER, t0);
    return PGRC_OK;
}

// orgIdx2PgPos in s->pos (T positions of eight bytes) with the proof that every index is written exactly once; on return the
// stream is idle and ev[1] recorded.  Shared by pgrc_rlist_pair_positions and pgrc_rlist_positions (`who`)
static int rl_positions_build(pgrc_rlist *s, const pgrc_rlist_pairpos_args *x, const std::string &who) {
    const uint64_t T = x->n_total;
    pgrc_match_ctx *c = x->matcher;
    int e;
    pgrc_rlist *const lists[3] = {x->hq, x->lq, x->n};
    const uint64_t base[3] = {0, x->hq_len, x->hq_len + x->lq_len};
    uint64_t longest = c ? c->rd.n + 1 : 1, writers = 0;
    for (pgrc_rlist *l : lists)
        if (l) {
            longest = std::max(longest, l->cur.n);
            writers += l->cur.n;
        }
    if ((e = pgrc_bufs_unpooled(s, {{&s->pos, T * 8 + 16}, {&s->cls, T + 16}, {&s->words, 64}, {&s->scan, longest * 8 + 16}}))) return e;
    uint64_t *pos = (uint64_t *)s->pos.p;
    uint8_t *cls = (uint8_t *)s->cls.p;
    uint32_t *bad = (uint32_t *)s->words.p;
    // the matcher's results and the reads' original indexes
    const uint32_t *d_rorg = nullptr;
    const uint64_t *d_mpos = nullptr;
    uint64_t matched = 0;
    if (c) {
        if (x->sets) {
            if ((e = rl_reads_org(s, x->sets, c->rd.n, who.c_str(), &d_rorg))) return e;
        } else if (x->read_org_idx) {
            if ((e = pgrc_buf_unpooled(s, s->map, c->rd.n * 4 + 16)) || (e = dec_upload_host(s, s->map.p, x->read_org_idx, c->rd.n * 4))) return e;
            s->tm.bytes_up = c->rd.n * 4;
            d_rorg = (const uint32_t *)s->map.p;
        }
        HIP_TRY(s, hipEventRecord(s->ev_x[0], c->stream));
        HIP_TRY(s, hipStreamWaitEvent(s->stream, s->ev_x[0], 0));
        d_mpos = (const uint64_t *)c->res.d_pos.p;
        if ((e = dec_scan<false>(s, XfBelow{d_mpos, PGRC_NOT_MATCHED_POS}, c->rd.n, 0, (uint64_t *)s->scan.p))) return e;
        HIP_TRY(s, hipMemcpyAsync(&matched, (const uint64_t *)s->scan.p + c->rd.n, 8, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(s, hipStreamSynchronize(s->stream));
        writers += matched;
    }
    // nothing is launched for an input that cannot write every index once
    if (writers != T)
        return rl_fail(s, PGRC_E_PARAM, who + ": the lists and the matched reads are " + std::to_string(writers) + ", n_total is " + std::to_string(T) +
                                            (writers > T ? ": an index is written twice" : ": an index is never written"));
    if (T) HIP_TRY(s, hipMemsetAsync(pos, 0xFF, T * 8, s->stream));      // vector<uint_pg_len_max>(readsTotalCount, -1)
    if (T) HIP_TRY(s, hipMemsetAsync(cls, 0, T, s->stream));
    HIP_TRY(s, hipMemsetAsync(bad, 0, 64, s->stream));
    if ((e = pgrc_buf_unpooled(s, s->scratch, sco_scratch_elems(longest) * sizeof(uint64_t)))) return e;
    for (int pass = 0; pass < 2; pass++) {
        for (int l = 0; l < 3; l++) {
            if (!lists[l] || !lists[l]->cur.n) continue;
            const RlBufs &b = lists[l]->cur;
            const RlPosOut o{(const uint32_t *)b.org.p, T, pos, cls, bad, (uint8_t)(l + 1), pass == 1};
            HIP_TRY(s, (sco_device_scan<true, false>(s->stream, XfU16{(const uint16_t *)b.off.p}, b.n, ScoPlus{}, (uint64_t)0, base[l], o, (uint64_t *)s->scratch.p)));
        }
        if (c && c->rd.n) hipLaunchKernelGGL(k_rl_pos_matched, dim3(rl_grid(c->rd.n)), dim3(RL_TPB), 0, s->stream, d_mpos, c->rd.n, d_rorg, T, pass == 1, pos, cls, bad);
        HIP_TRY(s, hipGetLastError());
    }
    if (T) hipLaunchKernelGGL(k_rl_pos_never, dim3(rl_grid(T)), dim3(RL_TPB), 0, s->stream, (const uint8_t *)cls, T, bad);
    HIP_TRY(s, hipGetLastError());
    HIP_TRY(s, s->ev.record(1, s->stream));
    uint32_t h_bad[RL_BAD_WORDS] = {};
    HIP_TRY(s, hipMemcpyAsync(h_bad, bad, sizeof h_bad, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    if (h_bad[RL_BAD_RANGE]) return rl_fail(s, PGRC_E_PARAM, who + ": an original index of " + std::to_string(T) + " (n_total) or more");
    if (h_bad[RL_BAD_TWICE] || h_bad[RL_BAD_NEVER]) return rl_fail(s, PGRC_E_PARAM, who + ": an index is written twice and another never");
    return PGRC_OK;
}

static int rl_pair_positions(pgrc_rlist *s, const pgrc_rlist_pairpos_args *x, pgrc_pairpos_streams *out) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t T = x->n_total;
    int e;
    if ((e = rl_begin(s)) || (e = rl_positions_build(s, x, "pair_positions"))) return e;
    if ((e = pgrc_pairpos_encode_device(s, s->pp, (const uint64_t *)s->pos.p, T, x->pos_width, out))) return e;
    for (int k = 2; k < 4; k++) HIP_TRY(s, s->ev.record(k, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    s->tm.bytes_down = s->pp.tm.bytes_down;
    rl_done(s, PGRC_RLIST_PAIR_POSITIONS, t0);
    return PGRC_OK;
}

// the array narrowed to pos_width bytes on the device and brought down in one block
static int rl_positions(pgrc_rlist *s, const pgrc_rlist_pairpos_args *x, pgrc_rlist_positions_out *out) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t T = x->n_total, W = x->pos_width;
    int e;
    if ((e = rl_begin(s)) || (e = rl_positions_build(s, x, "positions"))) return e;
    HIP_TRY(s, s->ev.record(2, s->stream));
    const void *d_out = s->pos.p;
    if (W == 4) {
        uint32_t *bad = (uint32_t *)s->words.p;       // (all zero: the build has returned)
        if ((e = pgrc_buf_unpooled(s, s->block, T * 4 + 16))) return e;
        if (T) hipLaunchKernelGGL(k_rl_pos_narrow, dim3(rl_grid(T)), dim3(RL_TPB), 0, s->stream, (const uint64_t *)s->pos.p, T, (uint32_t *)s->block.p, bad);
        HIP_TRY(s, hipGetLastError());
        uint32_t h_bad[RL_BAD_WORDS] = {};
        HIP_TRY(s, hipMemcpyAsync(h_bad, bad, sizeof h_bad, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(s, hipStreamSynchronize(s->stream));
        if (h_bad[RL_BAD_WIDE]) return rl_fail(s, PGRC_E_PARAM, "positions: a position of 2^32 or more with pos_width 4");
        d_out = s->block.p;
    }
    HIP_TRY(s, s->ev.record(3, s->stream));
    const uint64_t bytes[1] = {T * W};
    const void *src[1] = {d_out};
    uint8_t *blk = nullptr;
    uint64_t down = 0;
    if ((e = dec_download_block(s, "reads list: positions", dec_block_layout(bytes), src, &blk, &down))) return e;
    out->struct_size = sizeof(pgrc_rlist_positions_out);
    out->pos_width = (uint32_t)W;
    out->n_total = T;
    out->positions = blk;
    out->block_bytes = down;
    out->block = blk;
    s->tm.bytes_down = down;
    rl_done(s, PGRC_RLIST_POSITIONS, t0);
    return PGRC_OK;
}

extern "C" {

const char *pgrc_rlist_last_error(const pgrc_rlist *s) { return s ? s->err.c_str() : g_rl_create_err.c_str(); }

int pgrc_rlist_create(int32_t device, pgrc_rlist **out) {
    if (!out) return PGRC_E_PARAM;
    *out = nullptr;
    pgrc_rlist *s = new pgrc_rlist();
    const int e = pgrc_stage_open(s, device, &g_rl_create_err);
    if (e) {
        g_rl_create_err = "reads list: " + g_rl_create_err;
        delete s;
        return e;
    }
    *out = s;
    return PGRC_OK;
}

void pgrc_rlist_destroy(pgrc_rlist *s) {
    if (!s) return;
    {
        PgrcDeviceScope scope(s->device);
        (void)hipStreamSynchronize(s->stream);
        rl_free(s->cur);
        dec_free_all(rl_bufs(s));
        s->la.release();
        s->po.release();
        s->pp.release();
        s->ev.release();
        for (hipEvent_t ev : s->ev_x)
            if (ev) (void)hipEventDestroy(ev);
    }
    pgrc_stage_close(s);
    delete s;
}

int pgrc_rlist_get_info(pgrc_rlist *s, pgrc_rlist_info *out) {
    if (!s) return PGRC_E_PARAM;
    if (!out || out->struct_size != sizeof(pgrc_rlist_info)) return rl_fail(s, PGRC_E_PARAM, "info is NULL or struct_size is not sizeof(pgrc_rlist_info)");
    *out = pgrc_rlist_info{};
    out->struct_size = sizeof(pgrc_rlist_info);
    out->off_width = s->cur.off_width;
    out->n_entries = s->cur.n;
    out->n_mismatches = s->cur.nmis;
    out->last_pos = s->cur.last_pos;
    out->has_rev_comp = s->cur.has_rc;
    out->has_mismatches = s->cur.has_mis;
    return PGRC_OK;
}

int pgrc_rlist_get_timing(pgrc_rlist *s, pgrc_rlist_timing *out) {
    if (!s) return PGRC_E_PARAM;
    if (!out || out->struct_size != sizeof(pgrc_rlist_timing)) return rl_fail(s, PGRC_E_PARAM, "timing is NULL or struct_size is not sizeof(pgrc_rlist_timing)");
    if (!s->have_timing) return rl_fail(s, PGRC_E_STATE, "no call has succeeded on this object");
    *out = s->tm;
    return PGRC_OK;
}

int pgrc_rlist_set_host(pgrc_rlist *s, const pgrc_export_streams *in) {
    if (!s) return PGRC_E_PARAM;
    if (!in) return rl_fail(s, PGRC_E_PARAM, "set_host: in is NULL");
    if (in->n_entries >= (1ull << 32) || in->n_mismatches >= (1ull << 32)) return rl_fail(s, PGRC_E_PARAM, "set_host: 2^32 entries or mismatches or more");
    if (in->off_width != 1 && in->off_width != 2) return rl_fail(s, PGRC_E_PARAM, "set_host: off_width must be 1 or 2");
    if (in->n_entries && (!in->off || !in->org_idx)) return rl_fail(s, PGRC_E_PARAM, "set_host: off or org_idx is NULL with a non-zero count");
    // the list carries mismatch streams if the three are given (a stream without an element is given too), none if none is
    const int have = (in->mis_cnt != nullptr) + (in->mis_sym != nullptr) + (in->mis_rev_off != nullptr);
    if (have != 0 && have != 3) return rl_fail(s, PGRC_E_PARAM, "set_host: the mismatch streams are all present or all absent");
    const bool mis = have == 3;
    if (!mis && in->n_mismatches) return rl_fail(s, PGRC_E_PARAM, "set_host: n_mismatches without the mismatch streams");
    PGRC_ON_DEVICE(s);
    return rl_set_host(s, in);
}

int pgrc_rlist_from_assembly(pgrc_rlist *s, pgrc_asm_ctx *a, pgrc_rsets *sets, int32_t which) {
    if (!s) return PGRC_E_PARAM;
    if (!a) return rl_fail(s, PGRC_E_PARAM, "from_assembly: the assembly context is NULL");
    PgasmLastList l;
    pgasm_last_list(a, &l);
    if (l.device != s->device) return rl_fail(s, PGRC_E_PARAM, "from_assembly: the assembly context is on another device");
    if (sets && sets->device != s->device) return rl_fail(s, PGRC_E_PARAM, "from_assembly: the read sets are on another device");
    if (sets && (which < PGRC_RSETS_HQ || which > PGRC_RSETS_N)) return rl_fail(s, PGRC_E_PARAM, "from_assembly: which is PGRC_RSETS_HQ, PGRC_RSETS_LQ or PGRC_RSETS_N");
    if (!l.valid) return rl_fail(s, PGRC_E_STATE, "from_assembly: no run has succeeded on the assembly context");
    if (sets && l.mapped) return rl_fail(s, PGRC_E_STATE, "from_assembly: the assembly run has applied a host mapping already");
    const uint32_t *d_map = nullptr;
    uint64_t count = 0;
    int e;
    if (sets && (e = pgrc_rsets_mapping_device(sets, which, &d_map, &count))) return rl_fail(s, e, std::string("from_assembly: ") + pgrc_rsets_last_error(sets));
    PGRC_ON_DEVICE(s);
    return rl_from_assembly(s, l, d_map, count);
}

int pgrc_rlist_from_overlap(pgrc_rlist *s, pgrc_ovl_ctx *ovl, pgrc_asm_ctx *a, pgrc_rsets *sets, int32_t which, pgrc_asm_result *res) {
    if (!s) return PGRC_E_PARAM;
    if (res) *res = pgrc_asm_result{};
    if (!ovl || !a || !res) return rl_fail(s, PGRC_E_PARAM, "from_overlap: the overlap context, the assembly context or the result is NULL");
    if (pgovl_device(ovl) != s->device) return rl_fail(s, PGRC_E_PARAM, "from_overlap: the overlap context is on another device");
    int e;
    if ((e = pgovl_assemble(ovl, a, nullptr, res, true))) return rl_fail(s, e, std::string("from_overlap: ") + pgrc_ovl_last_error(ovl));
    if ((e = pgrc_rlist_from_assembly(s, a, sets, which))) *res = pgrc_asm_result{};
    return e;
}

int pgrc_rlist_export_pg_order(pgrc_rlist *s, pgrc_match_ctx *c, const pgrc_rlist_export_args *x) {
    if (!s) return PGRC_E_PARAM;
    if (!c) return rl_fail(s, PGRC_E_PARAM, "export_pg_order: the matcher is NULL");
    if (!x || x->struct_size != sizeof(pgrc_rlist_export_args)) return rl_fail(s, PGRC_E_PARAM, "export_pg_order: args is NULL or struct_size is not sizeof(pgrc_rlist_export_args)");
    if (x->sets && x->read_org_idx) return rl_fail(s, PGRC_E_PARAM, "export_pg_order: the reads' original indexes are given twice (read_org_idx and sets)");
    int e;
    if ((e = rl_matcher_ok(s, c, "export_pg_order"))) return e;
    if (s->cur.has_mis) return rl_fail(s, PGRC_E_STATE, "export_pg_order: the list carries mismatches already");
    PGRC_ON_DEVICE(s);
    if ((e = rl_export(s, c, x))) (void)hipStreamSynchronize(s->stream);
    return e;
}

int pgrc_rlist_download(pgrc_rlist *s, pgrc_export_streams *out) {
    if (!s) return PGRC_E_PARAM;
    if (!out) return rl_fail(s, PGRC_E_PARAM, "download: out is NULL");
    memset(out, 0, sizeof *out);
    PGRC_ON_DEVICE(s);
    const int e = rl_download_run(s, out);
    if (e) {
        (void)hipStreamSynchronize(s->stream);
        pgrc_match_free_export(out);
    }
    return e;
}

int pgrc_rlist_archive_encode(pgrc_rlist *s, int32_t fast_level, int32_t want_org_idx, pgrc_rlist_archive *out) {
    if (!s) return PGRC_E_PARAM;
    if (!out) return rl_fail(s, PGRC_E_PARAM, "archive_encode: out is NULL");
    *out = pgrc_rlist_archive{};
    if (s->cur.has_mis && s->cur.off_width != 1)
        return rl_fail(s, PGRC_E_PARAM, "archive_encode: offsets of " + std::to_string(s->cur.off_width) + " bytes (the archive's loader reads one byte each)");
    PGRC_ON_DEVICE(s);
    const int e = rl_archive(s, fast_level != 0, want_org_idx != 0, false, out);
    if (e) {
        (void)hipStreamSynchronize(s->stream);
        *out = pgrc_rlist_archive{};
    }
    return e;
}

void pgrc_rlist_archive_free(pgrc_rlist_archive *a) {
    if (!a) return;
    if (a->block) (void)hipHostFree(a->block);
    *a = pgrc_rlist_archive{};
}

int pgrc_rlist_pair_order(pgrc_rlist *const lists[3], int32_t form, pgrc_pairorder_streams *out) {
    if (!lists) return PGRC_E_PARAM;
    pgrc_rlist *s = lists[0] ? lists[0] : lists[1] ? lists[1] : lists[2];
    if (!s) return PGRC_E_PARAM;
    if (!out) return rl_fail(s, PGRC_E_PARAM, "pair_order: out is NULL");
    *out = pgrc_pairorder_streams{};
    uint64_t T = 0;
    for (int l = 0; l < 3; l++) {
        if (!lists[l]) continue;
        if (lists[l]->device != s->device) return rl_fail(s, PGRC_E_PARAM, "pair_order: the lists are on different devices");
        T += lists[l]->cur.n;
    }
    PGRC_ON_DEVICE(s);
    const int e = rl_pair_order(s, lists, T, form, out);
    if (e) (void)hipStreamSynchronize(s->stream);
    return e;
}

// what both position calls check of their arguments (x->hq is there)
static int rl_positions_args_ok(const pgrc_rlist_pairpos_args *x, const std::string &who) {
    pgrc_rlist *s = x->hq;
    if (x->struct_size != sizeof(pgrc_rlist_pairpos_args)) return rl_fail(s, PGRC_E_PARAM, who + ": struct_size is not sizeof(pgrc_rlist_pairpos_args)");
    if (x->sets && x->read_org_idx) return rl_fail(s, PGRC_E_PARAM, who + ": the reads' original indexes are given twice (read_org_idx and sets)");
    for (pgrc_rlist *l : {x->lq, x->n})
        if (l && l->device != s->device) return rl_fail(s, PGRC_E_PARAM, who + ": the lists are on different devices");
    int e;
    if (x->matcher) {
        if ((e = rl_matcher_ok(s, x->matcher, who.c_str()))) return e;
        if (!x->matcher->res.have_results || !x->matcher->res.d_pos.p) return rl_fail(s, PGRC_E_STATE, who + ": the matcher has no results");
    }
    return PGRC_OK;
}

int pgrc_rlist_pair_positions(const pgrc_rlist_pairpos_args *x, pgrc_pairpos_streams *out) {
    if (!x || !x->hq) return PGRC_E_PARAM;
    pgrc_rlist *s = x->hq;
    if (x->struct_size != sizeof(pgrc_rlist_pairpos_args)) return rl_fail(s, PGRC_E_PARAM, "pair_positions: struct_size is not sizeof(pgrc_rlist_pairpos_args)");
    if (!out) return rl_fail(s, PGRC_E_PARAM, "pair_positions: out is NULL");
    *out = pgrc_pairpos_streams{};
    int e;
    if ((e = rl_positions_args_ok(x, "pair_positions"))) return e;
    PGRC_ON_DEVICE(s);
    if ((e = rl_pair_positions(s, x, out))) {
        (void)hipStreamSynchronize(s->stream);
        *out = pgrc_pairpos_streams{};
    }
    return e;
}

}   // extern "C"

// ------------------------------------------------------------------------------------------------ the order-preserving mode
// The entry points of include/pgrc_readslist_ord.h (rlistord.hip exports them from a library of its own)
int pgrc_rl_export_original_order(pgrc_rlist *s, pgrc_match_ctx *c, const pgrc_rlist_export_org_args *x) {
    if (!s) return PGRC_E_PARAM;
    if (!c) return rl_fail(s, PGRC_E_PARAM, "export_original_order: the matcher is NULL");
    if (!x || x->struct_size != sizeof(pgrc_rlist_export_org_args))
        return rl_fail(s, PGRC_E_PARAM, "export_original_order: args is NULL or struct_size is not sizeof(pgrc_rlist_export_org_args)");
    if (x->sets && x->read_org_idx) return rl_fail(s, PGRC_E_PARAM, "export_original_order: the reads' original indexes are given twice (read_org_idx and sets)");
    int e;
    if ((e = rl_matcher_ok(s, c, "export_original_order"))) return e;
    if (c->rd.n && !x->sets && !x->read_org_idx) return rl_fail(s, PGRC_E_PARAM, "export_original_order: neither read_org_idx nor sets");
    PGRC_ON_DEVICE(s);
    if ((e = rl_export_org(s, c, x))) (void)hipStreamSynchronize(s->stream);
    return e;
}

int pgrc_rl_archive_encode_ord(pgrc_rlist *s, int32_t fast_level, pgrc_rlist_archive *out) {
    if (!s) return PGRC_E_PARAM;
    if (!out) return rl_fail(s, PGRC_E_PARAM, "archive_encode_ord: out is NULL");
    *out = pgrc_rlist_archive{};
    if (!s->cur.has_rc || !s->cur.has_mis) return rl_fail(s, PGRC_E_STATE, "archive_encode_ord: the list has no RC flags or no mismatch streams (export_original_order makes them)");
    if (s->cur.off_width != 1)
        return rl_fail(s, PGRC_E_PARAM, "archive_encode_ord: offsets of " + std::to_string(s->cur.off_width) + " bytes (the archive's loader reads one byte each)");
    PGRC_ON_DEVICE(s);
    const int e = rl_archive(s, fast_level != 0, false, true, out);
    if (e) {
        (void)hipStreamSynchronize(s->stream);
        *out = pgrc_rlist_archive{};
    }
    return e;
}

int pgrc_rl_positions(const pgrc_rlist_pairpos_args *x, pgrc_rlist_positions_out *out) {
    if (!x || !x->hq) return PGRC_E_PARAM;
    pgrc_rlist *s = x->hq;
    if (!out || out->struct_size != sizeof(pgrc_rlist_positions_out)) return rl_fail(s, PGRC_E_PARAM, "positions: out is NULL or struct_size is not sizeof(pgrc_rlist_positions_out)");
    *out = pgrc_rlist_positions_out{};
    int e;
    if ((e = rl_positions_args_ok(x, "positions"))) return e;
    if (x->pos_width != 4 && x->pos_width != 8) return rl_fail(s, PGRC_E_PARAM, "positions: pos_width must be 4 or 8");
    PGRC_ON_DEVICE(s);
    if ((e = rl_positions(s, x, out))) {
        (void)hipStreamSynchronize(s->stream);
        *out = pgrc_rlist_positions_out{};
    }
    return e;
}

void pgrc_rl_positions_free(pgrc_rlist_positions_out *o) {
    if (!o) return;
    if (o->block) (void)hipHostFree(o->block);
    *o = pgrc_rlist_positions_out{};
}
