// decode.hip -- the rebuild of the reads from the pseudogenomes and their reads lists (include/pgrc_decode.h): the inverse
// of the export (export.hip).
//
// Reference behaviour restated (not translated):
//   SeparatedPseudoGenome::getRead / getRead_Unsafe / getNextRead_*   pseudogenome/SeparatedPseudoGenome.cpp:74-120
//   enableConstantAccess (positions, mismatch list starts)             pseudogenome/readslist/SeparatedExtendedReadsList.cpp:328-363
//   convertMisRevOffsets2Offsets                                       utils/helper.h:52-63
//   code2mismatch, reverseComplementInPlace, complementsLut            utils/helper.cpp:243-262, :353-356, :383-393
//   writeAllReadsInSEMode* / PEMode* / ORDMode*                        pgrc/pgrc-decoder.cpp:137-527
//   applyRevComplPairFileToPgs                                         pgrc/pgrc-decoder.cpp:700-724
//
// The reference decodes serially per 128 KiB chunk on at most 4 threads (pgrc-decoder.h:34-35).  Here:
//   entry tables  positions = inclusive scan of the widened offset deltas, list starts = exclusive scan of the mismatch
//                 counts, forward mismatch offsets per entry (k_dec_mis), the ORD rank over "position < hqPgLen"
//   row kernel    a workgroup assembles a tile of R consecutive output rows in LDS (R*(L+1) a multiple of 16): the
//                 windows come from ONE coalesced load of the tile's text span when it fits (SE order: positions
//                 ascend), else from per-row 16-byte gathers; RC and mismatches are applied in LDS; the tile leaves as
//                 16-byte stores per lane
//   download      rows are made into a device chunk and copied down while the next chunk is made (two chunks)
#include <chrono>

#include "decctx.h"

#define DEC_RMAX 256            // rows per tile at most (per-row LDS arrays)
#define DEC_TILE_TARGET 8192    // bytes of a tile, about
#define DEC_SRC_CAP 16384       // LDS bytes for the windows: a tile's text span, or its rows' gathered 16-byte lines
#define DEC_TILE_CAP 12288      // R*(L+1) < DEC_TILE_TARGET + 16*(L+1) <= 12288
#define DEC_CHUNK_BYTES (64ull << 20)

struct DecList {                // device view of one list (kernel argument)
    const uint64_t *pos;        // joined-text positions, NULL = none
    const uint8_t *rc;          // NULL = revComp disabled
    const uint64_t *mcum;       // n+1 mismatch list starts, NULL = mismatches disabled
    const uint8_t *moff;        // forward mismatch offsets
    const uint8_t *msym;        // form 1: the mismatch symbol itself; form 0: the exclusive code
    uint64_t n, first_rl;
    uint32_t form;
    uint64_t order;             // val2sym after reorderSymAndVal, symbol v in byte v
};

struct DecArgs {
    const uint8_t *text;
    uint64_t text_len;
    DecList lst[3];
    uint32_t nl;
    uint32_t mode, file, pair;
    uint32_t L, L1, R;
    uint64_t first, n;          // rows of this launch: [first, first+n) of the file
    uint64_t n_entries;         // all lists
    const uint32_t *rl_order;   // PE
    const uint64_t *org2pos;    // ORD
    const uint64_t *rank;       // ORD: exclusive rank of the HQ rows
    uint64_t ord_base, half, hq_len;
    uint8_t *out;               // row `first` lands at out[0]
    uint32_t *err;
};

static thread_local std::string g_dec_create_err;

// ------------------------------------------------------------------------------------------------ entry tables
__global__ void k_dec_widen_pos(const uint64_t *__restrict__ in, uint64_t n, uint64_t base, uint64_t *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = in[i] + base;
}

// positions of four bytes, as the single-file ORD archive holds them for a joined text below 2^32, in the order's eight
__global__ void __launch_bounds__(256) k_dec_widen_u32(const uint32_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = in[i];
}

// every window inside the text: pos + L <= len
__global__ void k_dec_check_windows(const uint64_t *__restrict__ pos, uint64_t n, uint64_t lim, uint32_t *err) {
    uint32_t bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        bad |= pos[i] > lim;
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(err, DEC_F_WINDOW);
}

__global__ void k_dec_check_index(const uint32_t *__restrict__ idx, uint64_t n, uint64_t lim, uint32_t *err) {
    uint32_t bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        bad |= idx[i] >= lim;
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(err, DEC_F_INDEX);
}

// One thread per entry: the entry's mismatch offsets as forward offsets (convertMisRevOffsets2Offsets: the stream holds,
// for an entry of m mismatches, r_{m-1}, ..., r_0 with r_i = (the previous offset - 1, or L - 1) - off_i; so walking the
// stream, pos -= r + 1 yields off_{m-1}, ..., off_0), and the codes checked and, in the context form, turned into the
// mismatch symbol itself (cxtCode2Mismatch under the default order, helper.cpp:371-374).
template <typename OffT>
__global__ void k_dec_mis(const uint64_t *__restrict__ mcum, uint64_t n, const OffT *__restrict__ off_in, const uint8_t *__restrict__ sym_in,
                          uint32_t L, int rev_coded, uint32_t form, uint8_t *__restrict__ moff, uint8_t *__restrict__ msym, uint32_t *err) {
    uint32_t bad = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t s = mcum[e], m = mcum[e + 1] - s;
        int64_t p = L;
        for (uint64_t k = 0; k < m; k++) {
            int64_t o;
            uint64_t dst;
            if (rev_coded) {
                p -= (int64_t)off_in[s + k] + 1;
                o = p;
                dst = s + m - 1 - k;
            } else {
                o = off_in[s + k];
                dst = s + k;
            }
            if (o < 0 || o >= (int64_t)L) { bad |= DEC_F_MISOFF; o = 0; }
            moff[dst] = (uint8_t)o;
            const uint32_t c = sym_in[s + k];
            if (form) {
                if ((c & 15u) > 4u) bad |= DEC_F_MISSYM;
                msym[s + k] = (uint8_t)((0x4E54474341ull >> (8 * ((c & 15u) > 4u ? 4u : (c & 15u)))) & 0xFFu);   // "ACGTN"
            } else {
                if (c > 3u) bad |= DEC_F_MISSYM;
                msym[s + k] = (uint8_t)c;
            }
        }
    }
    if (bad) atomicOr(err, bad);
}

// ------------------------------------------------------------------------------------------------ the row kernel
__global__ void __launch_bounds__(DEC_TPB) k_dec_rows(DecArgs a) {
    __shared__ __align__(16) uint8_t s_src[DEC_SRC_CAP];
    __shared__ __align__(16) uint8_t s_tile[DEC_TILE_CAP];
    __shared__ uint64_t s_pos[DEC_RMAX];
    __shared__ uint64_t s_ms[DEC_RMAX];
    __shared__ uint32_t s_off[DEC_RMAX];
    __shared__ uint8_t s_mc[DEC_RMAX], s_rc[DEC_RMAX], s_list[DEC_RMAX];
    __shared__ uint8_t s_comp[256];
    __shared__ uint64_t s_red[2][DEC_TPB / 64];
    const uint32_t tid = threadIdx.x, L = a.L, L1 = a.L1;
    const uint64_t r0 = (uint64_t)blockIdx.x * a.R;
    const uint32_t nrows = (uint32_t)min((uint64_t)a.R, a.n - r0);
    s_comp[tid] = dec_complement(tid);

    // 1. entries: window position, RC flag, mismatch list of every row of the tile
    uint64_t pmin = ~0ull, pmax = 0;
    if (tid < nrows) {
        const uint64_t g = a.first + r0 + tid;
        uint32_t k = 0, rc = 0, bad = 0;
        uint64_t pos = 0, ms = 0, mc = 0;
        bool entry = true;
        uint64_t e = 0;
        if (a.mode == PGRC_DECODE_ORD) {
            const uint64_t i = a.ord_base + g;
            pos = a.org2pos[i];
            if (pos < a.hq_len) {
                e = a.rank[i];
                if (e >= a.lst[0].n) { bad |= DEC_F_INDEX; e = 0; entry = false; }
                rc = a.pair && i >= a.half;
            } else {
                entry = false;
                rc = a.file == 1;
            }
            if (entry) {
                if (a.lst[0].rc) rc ^= a.lst[0].rc[e];
                if (a.lst[0].mcum) { ms = a.lst[0].mcum[e]; mc = a.lst[0].mcum[e + 1] - ms; }
            }
        } else {
            uint64_t rl = g;
            if (a.mode == PGRC_DECODE_PE) rl = a.rl_order[2 * g + a.file];
            if (rl >= a.n_entries) { bad |= DEC_F_INDEX; rl = 0; }
            // (the list's fields by name, not by a run-time index into the argument struct: that would go through scratch)
            const uint64_t f1 = a.lst[1].first_rl, f2 = a.lst[2].first_rl;
            k = (a.nl > 1 && rl >= f1) ? ((a.nl > 2 && rl >= f2) ? 2 : 1) : 0;
            e = rl - (k == 0 ? 0 : k == 1 ? f1 : f2);
            const uint64_t *lp = k == 0 ? a.lst[0].pos : k == 1 ? a.lst[1].pos : a.lst[2].pos;
            if (lp) pos = lp[e];
            else bad |= DEC_F_NOPOS;
            if (k == 0) {
                const DecList &l = a.lst[0];
                if (l.rc) rc = l.rc[e];
                if (a.mode == PGRC_DECODE_PE && a.pair && a.file == 1) rc ^= 1;
                if (l.mcum) { ms = l.mcum[e]; mc = l.mcum[e + 1] - ms; }
            } else if (a.mode == PGRC_DECODE_PE) {
                rc = a.file == 1;      // LQ and N rows of file 2 are reverse-complemented (pgrc-decoder.cpp:275-276)
            }
        }
        if (a.text_len < L || pos > a.text_len - L) { bad |= DEC_F_WINDOW; pos = 0; mc = 0; }
        if (bad) atomicOr(a.err, bad);
        s_pos[tid] = pos;
        s_rc[tid] = (uint8_t)rc;
        s_ms[tid] = ms;
        s_mc[tid] = (uint8_t)min(mc, (uint64_t)255);
        s_list[tid] = (uint8_t)k;
        pmin = pos;
        pmax = pos;
    }
    // 2. the tile's span: min / max over the rows
    for (int o = 32; o > 0; o >>= 1) {
        pmin = min(pmin, (uint64_t)__shfl_xor(pmin, o, 64));
        pmax = max(pmax, (uint64_t)__shfl_xor(pmax, o, 64));
    }
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = pmin; s_red[1][tid >> 6] = pmax; }
    __syncthreads();
    for (uint32_t w = 0; w < DEC_TPB / 64; w++) { pmin = min(pmin, s_red[0][w]); pmax = max(pmax, s_red[1][w]); }
    const uint64_t span_lo = pmin & ~15ull;
    const uint64_t span_bytes = (pmax + L - span_lo + 15) & ~15ull;
    const uint4 *text16 = (const uint4 *)a.text;
    if (span_bytes <= DEC_SRC_CAP) {
        // 3a. one coalesced load of the span (the text is padded: the last 16-byte line stays inside the allocation)
        const uint64_t l0 = span_lo >> 4;
        for (uint32_t q = tid; q < (uint32_t)(span_bytes >> 4); q += DEC_TPB)
            ((uint4 *)s_src)[q] = text16[l0 + q];
        if (tid < nrows) s_off[tid] = (uint32_t)(s_pos[tid] - span_lo);
    } else {
        // 3b. per-row gathers: the 16-byte lines of every window, four in flight per lane
        const uint32_t lines = (L + 30) >> 4, stride = lines << 4;
        const uint32_t total = nrows * lines;
        auto line = [&](uint32_t q) -> uint4 {
            const uint32_t qq = q < total ? q : 0, row = qq / lines, c = qq - row * lines;
            return text16[(s_pos[row] >> 4) + c];
        };
        auto put = [&](uint32_t q, uint4 v) {
            const uint32_t row = q / lines, c = q - row * lines;
            if (q < total) ((uint4 *)s_src)[(row * stride >> 4) + c] = v;
        };
        for (uint32_t q0 = tid; q0 < total; q0 += 4 * DEC_TPB) {
            const uint4 v0 = line(q0), v1 = line(q0 + DEC_TPB), v2 = line(q0 + 2 * DEC_TPB), v3 = line(q0 + 3 * DEC_TPB);
            put(q0, v0);
            put(q0 + DEC_TPB, v1);
            put(q0 + 2 * DEC_TPB, v2);
            put(q0 + 3 * DEC_TPB, v3);
        }
        if (tid < nrows) s_off[tid] = tid * stride + (uint32_t)(s_pos[tid] & 15);
    }
    __syncthreads();
    // 4. the rows in the tile, 4 bytes per lane and step: the window, reversed and complemented for RC rows, '\n'
    const uint32_t tbytes = nrows * L1, twords = (tbytes + 3) >> 2;
    for (uint32_t w = tid; w < twords; w += DEC_TPB) {
        uint32_t b = w << 2, row = b / L1, col = b - row * L1, word = 0;
        for (int u = 0; u < 4 && b + u < tbytes; u++) {
            uint32_t c;
            if (col == L) c = '\n';
            else if (s_rc[row]) c = s_comp[s_src[s_off[row] + L - 1 - col]];
            else c = s_src[s_off[row] + col];
            word |= c << (8 * u);
            if (++col == L1) { col = 0; row++; }
        }
        ((uint32_t *)s_tile)[w] = word;
    }
    __syncthreads();
    // 5. mismatches, in list order, one lane per row (code2mismatch reads the symbol the row holds at that moment)
    if (tid < nrows && s_mc[tid]) {
        const DecList &l = a.lst[0];
        uint8_t *row = s_tile + tid * L1;
        const uint64_t s = s_ms[tid];
        for (uint32_t k = 0; k < s_mc[tid]; k++) {
            const uint32_t o = l.moff[s + k];
            const uint32_t c = l.msym[s + k];
            if (l.form) {
                row[o] = (uint8_t)c;
            } else {
                const uint32_t act = row[o];
                uint32_t av = 255;                       // sym2val of a byte outside the order: -1
                for (uint32_t v = 0; v < 5; v++)
                    if (((l.order >> (8 * v)) & 0xFFu) == act) av = v;
                row[o] = (uint8_t)(l.order >> (8 * (c < av ? c : c + 1)));
            }
        }
    }
    __syncthreads();
    // 6. the tile's bytes leave as 16-byte stores (the tile starts 16-byte aligned: r0 * (L+1) is a multiple of 16)
    uint8_t *dst = a.out + r0 * L1;
    const uint32_t full = tbytes >> 4;
    for (uint32_t q = tid; q < full; q += DEC_TPB)
        ((uint4 *)dst)[q] = ((const uint4 *)s_tile)[q];
    for (uint32_t b = (full << 4) + tid; b < tbytes; b += DEC_TPB)
        dst[b] = s_tile[b];
}

// ------------------------------------------------------------------------------------------------ host side
static uint32_t dec_rows_per_tile(uint32_t L) {
    const uint32_t L1 = L + 1;
    uint32_t g = 16;
    while (L1 % g) g >>= 1;
    const uint32_t R0 = 16 / g;                                        // R0 * (L+1) is a multiple of 16
    uint32_t R = R0 * std::max(1u, std::min(DEC_RMAX / R0, (DEC_TILE_TARGET + R0 * L1 - 1) / (R0 * L1)));
    const uint32_t stride = ((L + 30) >> 4) << 4;
    while (R > R0 && (R * stride > DEC_SRC_CAP || R * L1 > DEC_TILE_CAP)) R -= R0;
    return R;
}

static int dec_check_err(pgrc_decode_ctx *d, const char *what) {
    uint32_t f = 0;
    HIP_TRY(d, hipMemcpyAsync(&f, d->flag.p, 4, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    if (!f) return PGRC_OK;
    std::string m = std::string(what) + ":";
    if (f & DEC_F_WINDOW) m += " a window reaches past the text end;";
    if (f & DEC_F_INDEX) m += " an index out of range (rlIdx, or more HQ rows than HQ entries);";
    if (f & DEC_F_MISOFF) m += " a mismatch offset outside the read;";
    if (f & DEC_F_MISSYM) m += " a mismatch code outside its form's range;";
    if (f & DEC_F_NOPOS) m += " a row of a list without positions;";
    return dec_fail(d, PGRC_E_PARAM, m);
}

int pgrc_stage_open(PgrcStage *s, int32_t device, std::string *create_err) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        *create_err = "no HIP device";
        return PGRC_E_NO_DEVICE;
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess) { *create_err = "hipGetDevice failed"; return PGRC_E_NO_DEVICE; }
    if (device >= ndev) { *create_err = "device " + std::to_string(device) + " does not exist"; return PGRC_E_NO_DEVICE; }
    s->device = device;
    PgrcDeviceScope scope(device);
    int e = PGRC_OK;
    if (!scope.ok) e = PGRC_E_NO_DEVICE;
    if (!e && hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) e = PGRC_E_DEVICE;
    for (int k = 0; k < 2 && !e; k++)
        if (hipEventCreateWithFlags(&s->ev_copied[k], hipEventDisableTiming) != hipSuccess || hipHostMalloc((void **)&s->stage[k], DEC_STAGE_BYTES) != hipSuccess)
            e = PGRC_E_ALLOC;
    if (!e) e = pgrc_buf_unpooled(s, s->flag, 16);
    if (e) {
        *create_err = s->err.empty() ? "HIP stream / event / pinned buffer creation failed" : s->err;
        (void)hipGetLastError();
        pgrc_stage_close(s);
    }
    return e;
}

void pgrc_stage_close(PgrcStage *s) {
    PgrcDeviceScope scope(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    dec_free_all({&s->flag, &s->scratch});
    for (int k = 0; k < 2; k++) {
        if (s->stage[k]) (void)hipHostFree(s->stage[k]);
        if (s->ev_copied[k]) (void)hipEventDestroy(s->ev_copied[k]);
        s->stage[k] = nullptr;
        s->ev_copied[k] = nullptr;
    }
    if (s->stream) (void)hipStreamDestroy(s->stream);
    s->stream = nullptr;
}

// the decoder's own members on an open stage; the exported create adds the read length
int pgrc_decode_create_on(int32_t device, pgrc_decode_ctx **out) {
    *out = nullptr;
    pgrc_decode_ctx *d = new pgrc_decode_ctx();
    int e = pgrc_stage_open(d, device, &g_dec_create_err);
    if (e) {
        delete d;
        return e;
    }
    PgrcDeviceScope scope(d->device);
    if (hipStreamCreateWithFlags(&d->copy_stream, hipStreamNonBlocking) != hipSuccess) e = PGRC_E_DEVICE;
    for (int k = 0; k < 2 && !e; k++)
        if (hipEventCreate(&d->ev_made[k]) != hipSuccess || hipEventCreate(&d->ev_k0[k]) != hipSuccess) e = PGRC_E_ALLOC;
    if (!e && (hipEventCreate(&d->ev_a) != hipSuccess || hipEventCreate(&d->ev_b) != hipSuccess)) e = PGRC_E_DEVICE;
    if (e) {
        g_dec_create_err = "HIP stream / event / pinned buffer creation failed";
        (void)hipGetLastError();
        pgrc_decode_destroy(d);
        return e;
    }
    *out = d;
    return PGRC_OK;
}

static DevBufList dec_bufs(pgrc_decode_ctx *d) {
    DevBufList all = {&d->chunk[0], &d->chunk[1], &d->text, &d->rl_order, &d->org2pos, &d->rank, &d->rs_mapped, &d->rs_marks, &d->rs_vals, &d->rs_ptr, &d->rs_bsum,
                      &d->rs_coded, &d->rs_join};
    for (auto &l : d->lst) all.insert(all.end(), {&l.pos, &l.rc, &l.mcum, &l.moff, &l.msym, &l.raw});
    return all;
}

extern "C" {

int pgrc_decode_create(uint32_t read_length, int32_t device, pgrc_decode_ctx **out) {
    if (!out) return PGRC_E_PARAM;
    *out = nullptr;
    if (read_length < 1 || read_length > 255) { g_dec_create_err = "read length must be in [1, 255]"; return PGRC_E_PARAM; }
    const int e = pgrc_decode_create_on(device, out);
    if (!e) (*out)->L = read_length;
    return e;
}

void pgrc_decode_destroy(pgrc_decode_ctx *d) {
    if (!d) return;
    PgrcDeviceScope scope(d->device);
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    if (d->copy_stream) (void)hipStreamSynchronize(d->copy_stream);
    dec_free_all(dec_bufs(d));
    for (hipEvent_t ev : {d->ev_made[0], d->ev_made[1], d->ev_k0[0], d->ev_k0[1], d->ev_a, d->ev_b})
        if (ev) (void)hipEventDestroy(ev);
    d->pp.release();
    d->po.release();
    d->pod.release();
    d->la.release();
    if (d->copy_stream) (void)hipStreamDestroy(d->copy_stream);
    pgrc_stage_close(d);
    delete d;
}

const char *pgrc_decode_last_error(const pgrc_decode_ctx *d) { return d ? d->err.c_str() : g_dec_create_err.c_str(); }

int pgrc_decode_set_text(pgrc_decode_ctx *d, const char *joined, uint64_t len) {
    if (!d) return PGRC_E_PARAM;
    if (!joined && len) return dec_fail(d, PGRC_E_PARAM, "text is NULL");
    PGRC_ON_DEVICE(d);
    const auto t0 = std::chrono::steady_clock::now();
    d->have_text = false;
    d->have_parts = false;
    d->nl = 0;
    d->have_order = false;
    d->tm = pgrc_decode_timing{};
    const uint64_t bytes = ((len + 15) & ~15ull) + DEC_TEXT_PAD;
    int e;
    if ((e = pgrc_buf_unpooled(d, d->text, bytes))) return e;
    HIP_TRY(d, hipMemsetAsync((uint8_t *)d->text.p + (len & ~15ull), 0, bytes - (len & ~15ull), d->stream));
    if ((e = dec_upload(d, d->text.p, joined, len))) return e;
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    d->text_len = len;
    d->have_text = true;
    d->tm.ms_text = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PGRC_OK;
}

int pgrc_decode_add_list(pgrc_decode_ctx *d, const pgrc_decode_list *a) { return pgrc_dec_add_list(d, a, nullptr); }

}   // extern "C"

int pgrc_dec_add_list(pgrc_decode_ctx *d, const pgrc_decode_list *a, const pgrc_list_archive_streams *arch) {
    if (!d) return PGRC_E_PARAM;
    if (!a || a->struct_size != sizeof(pgrc_decode_list)) return dec_fail(d, PGRC_E_PARAM, "list is NULL or struct_size is not sizeof(pgrc_decode_list)");
    if (!d->have_text) return dec_fail(d, PGRC_E_STATE, "add_list before set_text");
    if (d->nl == 3) return dec_fail(d, PGRC_E_STATE, "three lists (HQ, LQ, N) are already added");
    if (arch && (a->mis_cnt || a->mis_sym || a->mis_off)) return dec_fail(d, PGRC_E_PARAM, "add_list_archive: the list's mis_* pointers must be NULL");
    if (d->nl > 0 && (a->rev_comp || a->mis_cnt || arch)) return dec_fail(d, PGRC_E_PARAM, "the LQ and N lists carry no RC flags and no mismatches");
    if (a->off && a->off_width != 1 && a->off_width != 2) return dec_fail(d, PGRC_E_PARAM, "off_width must be 1 or 2");
    const uint32_t mw = a->mis_off_width ? a->mis_off_width : (a->off ? a->off_width : 1);
    if (a->mis_cnt && (mw != 1 && mw != 2)) return dec_fail(d, PGRC_E_PARAM, "mis_off_width must be 1 or 2");
    if (a->mis_sym_form != 0 && a->mis_sym_form != 1) return dec_fail(d, PGRC_E_PARAM, "mis_sym_form must be 0 or 1");
    if (a->text_base > d->text_len) return dec_fail(d, PGRC_E_PARAM, "text_base beyond the text");
    const char *order = arch ? arch->bases_order : a->bases_order ? a->bases_order : "ACGTN";
    if (arch || (a->mis_cnt && !a->mis_sym_form)) {
        bool seen[256] = {};
        for (int v = 0; v < 5; v++) {
            if (seen[(uint8_t)order[v]]) return dec_fail(d, PGRC_E_PARAM, "bases_order repeats a symbol");
            seen[(uint8_t)order[v]] = true;
        }
    }
    const uint64_t n = a->n_entries;
    PGRC_ON_DEVICE(d);
    auto &l = d->lst[d->nl];          // (its device buffers, if an earlier text had a list here, are reused)
    l.has_pos = l.has_rc = l.has_mis = false;
    l.nmis = 0;
    l.n = n;
    l.text_base = a->text_base;
    l.form = arch ? 0u : (uint32_t)a->mis_sym_form;
    memcpy(l.order, order, 5);
    int e;
    if ((e = dec_clear_err(d))) return e;
    HIP_TRY(d, hipEventRecord(d->ev_a, d->stream));
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 4096));
    if (a->off || a->pos) {
        l.has_pos = true;
        if ((e = pgrc_buf_unpooled(d, l.pos, (n + 1) * 8))) return e;
        if (a->off) {
            if ((e = pgrc_buf_unpooled(d, l.raw, n * a->off_width + 16))) return e;
            if ((e = dec_upload(d, l.raw.p, a->off, n * a->off_width))) return e;
            if (a->off_width == 1) e = dec_scan<true>(d, XfU8{(const uint8_t *)l.raw.p}, n, a->text_base, (uint64_t *)l.pos.p);
            else e = dec_scan<true>(d, XfU16{(const uint16_t *)l.raw.p}, n, a->text_base, (uint64_t *)l.pos.p);
            if (e) return e;
        } else {
            if ((e = pgrc_buf_unpooled(d, l.raw, n * 8 + 16))) return e;
            if ((e = dec_upload(d, l.raw.p, a->pos, n * 8))) return e;
            if (n) hipLaunchKernelGGL(k_dec_widen_pos, dim3(grid), dim3(256), 0, d->stream, (const uint64_t *)l.raw.p, n, a->text_base, (uint64_t *)l.pos.p);
        }
        if (n) {
            if (d->text_len < d->L) HIP_TRY(d, hipMemsetAsync(d->flag.p, DEC_F_WINDOW, 1, d->stream));
            else hipLaunchKernelGGL(k_dec_check_windows, dim3(grid), dim3(256), 0, d->stream, (const uint64_t *)l.pos.p, n, d->text_len - d->L, (uint32_t *)d->flag.p);
        }
    }
    if (a->rev_comp) {
        l.has_rc = true;
        if ((e = pgrc_buf_unpooled(d, l.rc, n))) return e;
        if ((e = dec_upload(d, l.rc.p, a->rev_comp, n))) return e;
    }
    if (a->mis_cnt) {
        l.has_mis = true;
        if ((e = pgrc_buf_unpooled(d, l.raw, std::max<uint64_t>(n, 16)))) return e;
        if ((e = dec_upload(d, l.raw.p, a->mis_cnt, n))) return e;
        if ((e = pgrc_buf_unpooled(d, l.mcum, (n + 1) * 8))) return e;
        if ((e = dec_scan<false>(d, XfU8{(const uint8_t *)l.raw.p}, n, 0, (uint64_t *)l.mcum.p))) return e;
        uint64_t nm = 0;
        HIP_TRY(d, hipMemcpyAsync(&nm, (uint64_t *)l.mcum.p + n, 8, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(d, hipStreamSynchronize(d->stream));
        l.nmis = nm;
        if (nm && (!a->mis_sym || !a->mis_off)) return dec_fail(d, PGRC_E_PARAM, "mismatches counted but mis_sym / mis_off is NULL");
        // raw (reused): the codes, then the offsets at a 16-byte aligned place
        const uint64_t off_at = (nm + 15) & ~15ull;
        if ((e = pgrc_buf_unpooled(d, l.raw, off_at + nm * mw + 16)) || (e = pgrc_buf_unpooled(d, l.moff, nm)) || (e = pgrc_buf_unpooled(d, l.msym, nm))) return e;
        if ((e = dec_upload(d, l.raw.p, a->mis_sym, nm)) || (e = dec_upload(d, (uint8_t *)l.raw.p + off_at, a->mis_off, nm * mw))) return e;
        if (n) {
            const uint8_t *syms = (const uint8_t *)l.raw.p;
            if (mw == 1)
                hipLaunchKernelGGL((k_dec_mis<uint8_t>), dim3(grid), dim3(256), 0, d->stream, (const uint64_t *)l.mcum.p, n,
                                   (const uint8_t *)((uint8_t *)l.raw.p + off_at), syms, d->L, (int)a->mis_off_rev_coded, l.form,
                                   (uint8_t *)l.moff.p, (uint8_t *)l.msym.p, (uint32_t *)d->flag.p);
            else
                hipLaunchKernelGGL((k_dec_mis<uint16_t>), dim3(grid), dim3(256), 0, d->stream, (const uint64_t *)l.mcum.p, n,
                                   (const uint16_t *)((uint8_t *)l.raw.p + off_at), syms, d->L, (int)a->mis_off_rev_coded, l.form,
                                   (uint8_t *)l.moff.p, (uint8_t *)l.msym.p, (uint32_t *)d->flag.p);
        }
    }
    if (arch) {
        l.has_mis = true;
        if ((e = pgrc_la_tables(d, l, arch))) return e;
    }
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, hipEventRecord(d->ev_b, d->stream));
    if ((e = dec_check_err(d, arch ? "add_list_archive" : "add_list"))) return e;
    dec_free(l.raw);
    d->tm.ms_lists_device += dec_elapsed(d->ev_a, d->ev_b);
    d->nl++;
    d->have_order = false;
    return PGRC_OK;
}

extern "C" {

static uint64_t dec_entries(const pgrc_decode_ctx *d) {
    uint64_t t = 0;
    for (uint32_t k = 0; k < d->nl; k++) t += d->lst[k].n;
    return t;
}

// ORD: the checks of the T positions in d->org2pos (windows inside the text) and the ranks of the HQ rows
static int dec_ord_checks(pgrc_decode_ctx *d, uint64_t T) {
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((T + 255) / 256, 4096));
    const uint64_t hq_len = d->nl > 1 ? d->lst[1].text_base : d->text_len;
    int e;
    if (T) {
        if (d->text_len < d->L) HIP_TRY(d, hipMemsetAsync(d->flag.p, DEC_F_WINDOW, 1, d->stream));
        else hipLaunchKernelGGL(k_dec_check_windows, dim3(grid), dim3(256), 0, d->stream, (const uint64_t *)d->org2pos.p, T, d->text_len - d->L, (uint32_t *)d->flag.p);
    }
    if ((e = dec_scan<false>(d, XfBelow{(const uint64_t *)d->org2pos.p, hq_len}, T, 0, (uint64_t *)d->rank.p))) return e;
    uint64_t hq_rows = 0;
    HIP_TRY(d, hipMemcpyAsync(&hq_rows, (uint64_t *)d->rank.p + T, 8, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    if (hq_rows > d->lst[0].n) return dec_fail(d, PGRC_E_PARAM, "ORD order: more rows below hqPgLen than HQ entries");
    return PGRC_OK;
}

int pgrc_decode_set_order(pgrc_decode_ctx *d, const pgrc_decode_order *o) {
    if (!d) return PGRC_E_PARAM;
    if (!o || o->struct_size != sizeof(pgrc_decode_order)) return dec_fail(d, PGRC_E_PARAM, "order is NULL or struct_size is not sizeof(pgrc_decode_order)");
    if (!d->nl) return dec_fail(d, PGRC_E_STATE, "set_order before add_list");
    PGRC_ON_DEVICE(d);
    d->have_order = false;
    const uint64_t T = o->n_total;
    int e;
    if ((e = dec_clear_err(d))) return e;
    HIP_TRY(d, hipEventRecord(d->ev_a, d->stream));
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((T + 255) / 256, 4096));
    if (o->mode == PGRC_DECODE_SE) {
        if (o->rev_compl_pair_file) return dec_fail(d, PGRC_E_PARAM, "the pair-file rule needs PE or ORD order");
    } else if (o->mode == PGRC_DECODE_PE) {
        if (!o->rl_idx_order && T) return dec_fail(d, PGRC_E_PARAM, "PE order without rl_idx_order");
        if (T != dec_entries(d)) return dec_fail(d, PGRC_E_PARAM, "PE order: n_total differs from the lists' entries");
        if ((e = pgrc_buf_unpooled(d, d->rl_order, T * 4))) return e;
        if ((e = dec_upload(d, d->rl_order.p, o->rl_idx_order, T * 4))) return e;
        if (T) hipLaunchKernelGGL(k_dec_check_index, dim3(grid), dim3(256), 0, d->stream, (const uint32_t *)d->rl_order.p, T, dec_entries(d), (uint32_t *)d->flag.p);
    } else if (o->mode == PGRC_DECODE_ORD) {
        if (!o->org_idx_to_pos && T) return dec_fail(d, PGRC_E_PARAM, "ORD order without org_idx_to_pos");
        if ((e = pgrc_buf_unpooled(d, d->org2pos, T * 8)) || (e = pgrc_buf_unpooled(d, d->rank, (T + 1) * 8))) return e;
        if ((e = dec_upload(d, d->org2pos.p, o->org_idx_to_pos, T * 8))) return e;
        if ((e = dec_ord_checks(d, T))) return e;
    } else {
        return dec_fail(d, PGRC_E_PARAM, "unknown order mode");
    }
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, hipEventRecord(d->ev_b, d->stream));
    if ((e = dec_check_err(d, "set_order"))) return e;
    d->tm.ms_order_device = dec_elapsed(d->ev_a, d->ev_b);
    d->ord = *o;
    d->ord.rl_idx_order = nullptr;
    d->ord.org_idx_to_pos = nullptr;
    d->have_order = true;
    return PGRC_OK;
}

// The paired ORD order from the archive's own streams: the positions are decoded on the device (pairpos.hip) into org2pos
int pgrc_decode_set_order_pair_streams(pgrc_decode_ctx *d, const pgrc_pairpos_streams *s, int32_t rev_compl_pair_file) {
    if (!d) return PGRC_E_PARAM;
    d->have_order = false;
    int e;
    if ((e = pgrc_pairpos_check_streams(d, s))) return e;
    if (!d->nl) return dec_fail(d, PGRC_E_STATE, "set_order_pair_streams before add_list");
    PGRC_ON_DEVICE(d);
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t T = s->n_total;
    if ((e = pgrc_buf_unpooled(d, d->org2pos, T * 8)) || (e = pgrc_buf_unpooled(d, d->rank, (T + 1) * 8))) return e;
    if ((e = pgrc_pairpos_decode_device(d, s, (uint64_t *)d->org2pos.p))) return e;
    if ((e = dec_clear_err(d))) return e;
    HIP_TRY(d, hipEventRecord(d->ev_a, d->stream));
    if ((e = dec_ord_checks(d, T))) return e;
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, hipEventRecord(d->ev_b, d->stream));
    if ((e = dec_check_err(d, "set_order_pair_streams"))) return e;
    d->tm.ms_order_device = dec_elapsed(d->ev_a, d->ev_b);
    d->ord = pgrc_decode_order{};
    d->ord.struct_size = sizeof(pgrc_decode_order);
    d->ord.mode = PGRC_DECODE_ORD;
    d->ord.n_total = T;
    d->ord.paired = 1;
    d->ord.rev_compl_pair_file = rev_compl_pair_file;
    d->have_order = true;
    d->pp.tm.ms_download = 0;
    d->pp.tm.bytes_down = 0;
    d->pp.tm.ms_call = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    d->pp.have_timing = true;
    return PGRC_OK;
}

// The single-file ORD order from the archive's own array: positions of W bytes go up as they are; four-byte ones are staged
// in `rank` (the scan of dec_ord_checks fills it afterwards) and widened into org2pos
int pgrc_decode_set_order_positions(pgrc_decode_ctx *d, const void *positions, uint32_t pos_width, uint64_t n_total, int32_t rev_compl_pair_file) {
    if (!d) return PGRC_E_PARAM;
    d->have_order = false;
    if (pos_width != 4 && pos_width != 8) return dec_fail(d, PGRC_E_PARAM, "set_order_positions: pos_width must be 4 or 8");
    if (!positions && n_total) return dec_fail(d, PGRC_E_PARAM, "set_order_positions: positions is NULL with n_total > 0");
    if (!d->nl) return dec_fail(d, PGRC_E_STATE, "set_order_positions before add_list");
    PGRC_ON_DEVICE(d);
    const uint64_t T = n_total;
    int e;
    if ((e = pgrc_buf_unpooled(d, d->org2pos, T * 8)) || (e = pgrc_buf_unpooled(d, d->rank, (T + 1) * 8))) return e;
    if ((e = dec_clear_err(d))) return e;
    HIP_TRY(d, hipEventRecord(d->ev_a, d->stream));
    if (pos_width == 8) {
        if ((e = dec_upload(d, d->org2pos.p, positions, T * 8))) return e;
    } else {
        if ((e = dec_upload(d, d->rank.p, positions, T * 4))) return e;
        const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((T + 255) / 256, 4096));
        if (T) hipLaunchKernelGGL(k_dec_widen_u32, dim3(grid), dim3(256), 0, d->stream, (const uint32_t *)d->rank.p, T, (uint64_t *)d->org2pos.p);
        HIP_TRY(d, hipGetLastError());
    }
    if ((e = dec_ord_checks(d, T))) return e;
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, hipEventRecord(d->ev_b, d->stream));
    if ((e = dec_check_err(d, "set_order_positions"))) return e;
    d->tm.ms_order_device = dec_elapsed(d->ev_a, d->ev_b);
    d->ord = pgrc_decode_order{};
    d->ord.struct_size = sizeof(pgrc_decode_order);
    d->ord.mode = PGRC_DECODE_ORD;
    d->ord.n_total = T;
    d->ord.rev_compl_pair_file = rev_compl_pair_file;
    d->have_order = true;
    return PGRC_OK;
}

// The PE order from the archive's own streams: rlIdxOrder is decoded on the device (pairorder.hip) into rl_order
int pgrc_decode_set_order_pair_order_streams(pgrc_decode_ctx *d, const pgrc_pairorder_streams *s, int32_t rev_compl_pair_file) {
    if (!d) return PGRC_E_PARAM;
    d->have_order = false;
    int e;
    if ((e = pgrc_pairorder_check_streams(d, s))) return e;
    if (!d->nl) return dec_fail(d, PGRC_E_STATE, "set_order_pair_order_streams before add_list");
    PGRC_ON_DEVICE(d);
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t T = s->n_total;
    if (T != dec_entries(d)) return dec_fail(d, PGRC_E_PARAM, "PE order: n_total differs from the lists' entries");
    if ((e = pgrc_buf_unpooled(d, d->rl_order, T * 4))) return e;
    if ((e = pgrc_pairorder_decode_device(d, s, (uint32_t *)d->rl_order.p))) return e;
    if ((e = dec_clear_err(d))) return e;
    HIP_TRY(d, hipEventRecord(d->ev_a, d->stream));
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((T + 255) / 256, 4096));
    if (T) hipLaunchKernelGGL(k_dec_check_index, dim3(grid), dim3(256), 0, d->stream, (const uint32_t *)d->rl_order.p, T, dec_entries(d), (uint32_t *)d->flag.p);
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, hipEventRecord(d->ev_b, d->stream));
    if ((e = dec_check_err(d, "set_order_pair_order_streams"))) return e;
    d->tm.ms_order_device = dec_elapsed(d->ev_a, d->ev_b);
    d->ord = pgrc_decode_order{};
    d->ord.struct_size = sizeof(pgrc_decode_order);
    d->ord.mode = PGRC_DECODE_PE;
    d->ord.n_total = T;
    d->ord.rev_compl_pair_file = rev_compl_pair_file;
    d->have_order = true;
    d->pod.tm.ms_download = 0;
    d->pod.tm.bytes_down = 0;
    d->pod.tm.ms_call = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    d->pod.have_timing = true;
    return PGRC_OK;
}

static uint32_t dec_files(const pgrc_decode_ctx *d) {
    if (d->ord.mode == PGRC_DECODE_SE) return 1;
    if (d->ord.mode == PGRC_DECODE_PE) return 2;
    return d->ord.paired ? 2 : 1;
}

int pgrc_decode_row_count(pgrc_decode_ctx *d, uint32_t file, uint64_t *n_rows) {
    if (!d || !n_rows) return PGRC_E_PARAM;
    if (!d->have_order) return dec_fail(d, PGRC_E_STATE, "row_count before set_order");
    if (file >= dec_files(d)) return dec_fail(d, PGRC_E_PARAM, "no such output file");
    const uint64_t T = d->ord.n_total;
    if (d->ord.mode == PGRC_DECODE_SE) *n_rows = dec_entries(d);
    else if (d->ord.mode == PGRC_DECODE_PE) *n_rows = (T + 1 - file) / 2;          // i = file, file + 2, ... < T
    else *n_rows = T / (d->ord.paired ? 2 : 1);                                      // (readsTotalCount / parts) rows per file
    return PGRC_OK;
}

// the kernel arguments of rows [first, first+n) of `file`
static DecArgs dec_args(const pgrc_decode_ctx *d, uint32_t file, uint32_t R) {
    DecArgs a{};
    a.text = (const uint8_t *)d->text.p;
    a.text_len = d->text_len;
    uint64_t rl = 0;
    for (uint32_t k = 0; k < d->nl; k++) {
        const auto &l = d->lst[k];
        DecList &x = a.lst[k];
        x.pos = l.has_pos ? (const uint64_t *)l.pos.p : nullptr;
        x.rc = l.has_rc ? (const uint8_t *)l.rc.p : nullptr;
        x.mcum = l.has_mis ? (const uint64_t *)l.mcum.p : nullptr;
        x.moff = (const uint8_t *)l.moff.p;
        x.msym = (const uint8_t *)l.msym.p;
        x.n = l.n;
        x.first_rl = rl;
        x.form = l.form;
        x.order = 0;
        for (int v = 4; v >= 0; v--) x.order = (x.order << 8) | (uint8_t)l.order[v];
        rl += l.n;
    }
    a.nl = d->nl;
    a.n_entries = rl;
    a.mode = (uint32_t)d->ord.mode;
    a.file = file;
    a.pair = d->ord.rev_compl_pair_file ? 1 : 0;
    a.L = d->L;
    a.L1 = d->L + 1;
    a.R = R;
    a.rl_order = (const uint32_t *)d->rl_order.p;
    a.org2pos = (const uint64_t *)d->org2pos.p;
    a.rank = (const uint64_t *)d->rank.p;
    const uint64_t T = d->ord.n_total;
    a.half = T / 2;                                                     // pairsCount (pgrc-decoder.cpp:701)
    a.ord_base = (T / (d->ord.paired ? 2 : 1)) * file;
    a.hq_len = d->nl > 1 ? d->lst[1].text_base : d->text_len;
    a.err = (uint32_t *)d->flag.p;
    return a;
}

static int dec_launch(pgrc_decode_ctx *d, DecArgs a, uint64_t first, uint64_t n, void *d_out) {
    if (!n) return PGRC_OK;
    a.first = first;
    a.n = n;
    a.out = (uint8_t *)d_out;
    const uint64_t blocks = (n + a.R - 1) / a.R;
    hipLaunchKernelGGL(k_dec_rows, dim3((uint32_t)blocks), dim3(DEC_TPB), 0, d->stream, a);
    HIP_TRY(d, hipGetLastError());
    return PGRC_OK;
}

static int dec_rows_check(pgrc_decode_ctx *d, uint32_t file, uint64_t first, uint64_t n) {
    if (!d->have_order) return dec_fail(d, PGRC_E_STATE, "rows before set_order");
    uint64_t nr = 0;
    int e;
    if ((e = pgrc_decode_row_count(d, file, &nr))) return e;
    if (first > nr || n > nr - first) return dec_fail(d, PGRC_E_PARAM, "rows beyond the file's end");
    if (d->ord.mode != PGRC_DECODE_ORD)
        for (uint32_t k = 0; k < d->nl; k++)
            if (!d->lst[k].has_pos && d->lst[k].n) return dec_fail(d, PGRC_E_STATE, "a list without positions in SE / PE order");
    return PGRC_OK;
}

int pgrc_decode_rows_device(pgrc_decode_ctx *d, uint32_t file, uint64_t first, uint64_t n, void *d_out) {
    if (!d) return PGRC_E_PARAM;
    int e;
    if ((e = dec_rows_check(d, file, first, n))) return e;
    if (n && (!d_out || ((uintptr_t)d_out & 15))) return dec_fail(d, PGRC_E_PARAM, "d_out must be 16-byte aligned device memory");
    PGRC_ON_DEVICE(d);
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t R = dec_rows_per_tile(d->L);
    if ((e = dec_clear_err(d))) return e;
    HIP_TRY(d, hipEventRecord(d->ev_a, d->stream));
    // launches of at most 2^31 / R tiles (the grid's x limit)
    const uint64_t step = (uint64_t)R * (1ull << 30);
    const DecArgs a = dec_args(d, file, R);
    for (uint64_t o = 0; o < n; o += step)
        if ((e = dec_launch(d, a, first + o, std::min(step, n - o), (uint8_t *)d_out + o * (d->L + 1)))) return e;
    HIP_TRY(d, hipEventRecord(d->ev_b, d->stream));
    if ((e = dec_check_err(d, "rows"))) return e;
    d->tm.ms_rows_device = dec_elapsed(d->ev_a, d->ev_b);
    d->tm.rows_bytes = n * (d->L + 1);
    d->tm.ms_rows = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PGRC_OK;
}

int pgrc_decode_rows(pgrc_decode_ctx *d, uint32_t file, uint64_t first, uint64_t n, char *out) {
    if (!d) return PGRC_E_PARAM;
    int e;
    if ((e = dec_rows_check(d, file, first, n))) return e;
    if (n && !out) return dec_fail(d, PGRC_E_PARAM, "out is NULL");
    PGRC_ON_DEVICE(d);
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t R = dec_rows_per_tile(d->L), L1 = d->L + 1;
    const uint64_t crows = std::max<uint64_t>(R, DEC_CHUNK_BYTES / L1 / R * R);     // rows of one chunk: whole tiles
    const uint64_t cbytes = crows * L1;
    if ((e = pgrc_buf_unpooled(d, d->chunk[0], cbytes)) || (e = pgrc_buf_unpooled(d, d->chunk[1], cbytes))) return e;
    // pinned memory of the caller is written by the copy engine itself; other memory through the staging buffers
    const bool direct = pgrc_host_pinned(out);
    if (!direct && cbytes > DEC_STAGE_BYTES) return dec_fail(d, PGRC_E_PARAM, "internal: chunk above the staging size");
    if ((e = dec_clear_err(d))) return e;
    const DecArgs a = dec_args(d, file, R);
    float ms_k = 0;
    uint64_t pend_off = 0, pend_bytes = 0;     // staged: the chunk whose copy into stage[pend_k] is in flight
    int pend_k = -1;
    uint64_t nchunks = (n + crows - 1) / crows;
    for (uint64_t c = 0; c < nchunks; c++) {
        const int k = (int)(c & 1);
        const uint64_t r0 = c * crows, rn = std::min(crows, n - r0);
        if (c >= 2) {   // chunk c-2 used these buffers: its copy is done before the kernel overwrites them
            HIP_TRY(d, hipEventSynchronize(d->ev_copied[k]));
            ms_k += dec_elapsed(d->ev_k0[k], d->ev_made[k]);
        }
        HIP_TRY(d, hipEventRecord(d->ev_k0[k], d->stream));
        if ((e = dec_launch(d, a, first + r0, rn, d->chunk[k].p))) return e;
        HIP_TRY(d, hipEventRecord(d->ev_made[k], d->stream));
        HIP_TRY(d, hipStreamWaitEvent(d->copy_stream, d->ev_made[k], 0));
        void *dst = direct ? (void *)(out + r0 * L1) : (void *)d->stage[k];
        HIP_TRY(d, hipMemcpyAsync(dst, d->chunk[k].p, rn * L1, hipMemcpyDeviceToHost, d->copy_stream));
        HIP_TRY(d, hipEventRecord(d->ev_copied[k], d->copy_stream));
        if (!direct) {
            if (pend_k >= 0) {   // the previous chunk is down (or nearly): hand it over while this one is made and copied
                HIP_TRY(d, hipEventSynchronize(d->ev_copied[pend_k]));
                memcpy(out + pend_off, d->stage[pend_k], pend_bytes);
            }
            pend_k = k;
            pend_off = r0 * L1;
            pend_bytes = rn * L1;
        }
    }
    HIP_TRY(d, hipStreamSynchronize(d->copy_stream));
    if (pend_k >= 0) memcpy(out + pend_off, d->stage[pend_k], pend_bytes);
    for (uint64_t c = nchunks >= 2 ? nchunks - 2 : 0; c < nchunks; c++) ms_k += dec_elapsed(d->ev_k0[c & 1], d->ev_made[c & 1]);
    if ((e = dec_check_err(d, "rows"))) return e;
    d->tm.ms_rows_device = ms_k;
    d->tm.rows_bytes = n * L1;
    d->tm.ms_rows = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PGRC_OK;
}

int pgrc_decode_get_timing(pgrc_decode_ctx *d, pgrc_decode_timing *out) {
    if (!d || !out) return PGRC_E_PARAM;
    *out = d->tm;
    return PGRC_OK;
}

}   // extern "C"
