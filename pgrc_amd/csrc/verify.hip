// verify.hip -- include/pgrc_verify.h: a decode job checked against its source reads on the device.
//
// IN_ORDER streams: as source rows of a file arrive, the job's rows of the same range are made by decode.hip's row kernel
// (pgrc_decode_rows_device, on the job's stream, complete on return) into one of two chunks of the handle, and k_vf_compare
// reads both sides once: a power of two of lanes per row, 16 bytes a lane through aligned 8-byte loads, byte tails, one OR
// over the row's lanes, a block reduction, and per block one atomicAdd and one atomicMin.
//
// MULTISET keeps both sides.  k_vf_hash gives every item a 64-bit key,
//     key = fmix64(salt + sum over j of fmix64(w_j + (j + 1) * VF_K))        (all sums modulo 2^64)
// over the item's little-endian 8-byte words w_j, the last one zero-padded, fmix64 being MurmurHash3's finalizer: eight lanes
// take the words of an item in turn and add up, in any order.  The union of both sides' keys -- source first, the value an
// item's index with the side in bit 63 -- goes through radix.hip's stable sort once; head flags, a sum scan for the run
// number, the compaction of the head positions and a sum scan of the side bit (scanops.h through dec_scan) describe every
// run [a, b) of equal keys with cS source and cD decoded items; k_vf_confirm pairs offset o of either side with offset o of
// the other and compares the pair byte for byte, eight lanes a pair.  tests/verify_util.py restates the key bit for bit.
#include <atomic>

#include "verifyctx.h"

#define VF_TPB 256
#define VF_LPI 8                                    // lanes per item (k_vf_hash, k_vf_confirm)
#define VF_K 0x9E3779B97F4A7C15ull
#define VF_SALT_STEP 0xD6E8FEB86659FD93ull          // salt s is s * VF_SALT_STEP
#define VF_SIDE_BIT (1ull << 63)
#define VF_NONE (~0ull)
// the counters (unsigned long long[8])
#define VF_C_MATCHED 0
#define VF_C_UNDECIDED 1
#define VF_C_S_UNM 2
#define VF_C_D_UNM 3
#define VF_C_FIRST_S 4
#define VF_C_FIRST_D 5
#define VF_C_ROWS 6
#define VF_C_FIRST_ROW 7

static thread_local std::string g_vf_begin_err;
static std::atomic<uint32_t> g_vf_next_bits{0};

static int vf_fail(pgrc_verify *v, int code, const std::string &msg) { return dec_fail(v, code, "verify: " + msg); }

// ------------------------------------------------------------------------------------------------ device side
static __device__ __forceinline__ uint64_t vf_fmix64(uint64_t k) {
    k ^= k >> 33;
    k *= 0xFF51AFD7ED558CCDull;
    k ^= k >> 33;
    k *= 0xC4CEB9FE1A85EC53ull;
    k ^= k >> 33;
    return k;
}

static __device__ __forceinline__ uint64_t vf_shfl_xor(uint64_t v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}

// the 8 bytes at p, whatever its alignment, from aligned loads: up to 7 bytes behind p + 8 are read too (VF_PAD; every buffer
// starts 8-byte aligned, so nothing in front of it is)
static __device__ __forceinline__ uint64_t vf_load8(const uint8_t *p) {
    const uint64_t a = (uint64_t)p;
    const uint32_t sh = (uint32_t)(a & 7) * 8;
    const uint64_t *q = (const uint64_t *)(a & ~7ull);
    const uint64_t lo = q[0];
    if (!sh) return lo;
    return (lo >> sh) | (q[1] << (64 - sh));
}

// word j of an item: bytes [8 j, 8 j + 8) of file 0's row followed by file 1's, zeros behind the item's end
static __device__ __forceinline__ uint64_t vf_word(const VfSide &s, uint32_t F, uint32_t L, uint64_t item, uint32_t j) {
    const uint32_t o = j * 8, B = F * L;
    const uint32_t f = o >= L ? 1u : 0u, c = o - f * L;
    if (c + 8 <= L) return vf_load8(s.p[f] + item * s.stride[f] + c);
    uint64_t w = 0;
    for (uint32_t b = 0; b < 8 && o + b < B; b++) {
        const uint32_t ob = o + b, fb = ob >= L ? 1u : 0u;
        w |= (uint64_t)s.p[fb][item * s.stride[fb] + (ob - fb * L)] << (8 * b);
    }
    return w;
}

// sums and minima of the block's threads into the counters: no atomic where a block has nothing to say
template <int NS, int NM>
static __device__ __forceinline__ void vf_block_commit(uint64_t (&sum)[NS], uint64_t (&mn)[NM], unsigned long long *cnt, const int (&sum_at)[NS],
                                                        const int (&min_at)[NM]) {
    __shared__ uint64_t sm[VF_TPB / 64][NS + NM];
    for (int m = 32; m; m >>= 1) {
#pragma unroll
        for (int k = 0; k < NS; k++) sum[k] += vf_shfl_xor(sum[k], m);
#pragma unroll
        for (int k = 0; k < NM; k++) {
            const uint64_t u = vf_shfl_xor(mn[k], m);
            mn[k] = u < mn[k] ? u : mn[k];
        }
    }
    const uint32_t wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NS; k++) sm[wv][k] = sum[k];
#pragma unroll
        for (int k = 0; k < NM; k++) sm[wv][NS + k] = mn[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NS; k++) {
            uint64_t t = 0;
            for (int w = 0; w < VF_TPB / 64; w++) t += sm[w][k];
            if (t) atomicAdd(&cnt[sum_at[k]], (unsigned long long)t);
        }
#pragma unroll
        for (int k = 0; k < NM; k++) {
            uint64_t t = VF_NONE;
            for (int w = 0; w < VF_TPB / 64; w++) t = sm[w][NS + k] < t ? sm[w][NS + k] : t;
            if (t != VF_NONE) atomicMin(&cnt[min_at[k]], (unsigned long long)t);
        }
    }
}

static __global__ void k_vf_init_counts(unsigned long long *cnt) {
    if (threadIdx.x < 8) cnt[threadIdx.x] = (threadIdx.x == VF_C_FIRST_S || threadIdx.x == VF_C_FIRST_D || threadIdx.x == VF_C_FIRST_ROW) ? VF_NONE : 0ull;
}

// rows [0, n) of one file: src row r at src + r * sstride, rebuilt row r at dec + r * (L + 1); lpr lanes a row (a power of two,
// 16 * lpr >= L); row0: the file's row number of row 0
static __global__ void __launch_bounds__(VF_TPB) k_vf_compare(const uint8_t *__restrict__ src, uint64_t sstride, const uint8_t *__restrict__ dec, uint32_t L,
                                                             uint64_t n, uint64_t row0, uint32_t file, uint32_t lpr, unsigned long long *cnt) {
    const uint64_t t = (uint64_t)blockIdx.x * VF_TPB + threadIdx.x;
    const uint64_t row = t / lpr;
    const uint32_t o = (uint32_t)(t % lpr) * 16;
    uint32_t diff = 0;
    if (row < n && o < L) {
        const uint8_t *sp = src + row * sstride + o, *dp = dec + row * (uint64_t)(L + 1) + o;
        if (o + 16 <= L) {
            diff = ((vf_load8(sp) ^ vf_load8(dp)) | (vf_load8(sp + 8) ^ vf_load8(dp + 8))) != 0 ? 1u : 0u;
        } else {
            for (uint32_t b = 0; b < L - o; b++) diff |= sp[b] != dp[b] ? 1u : 0u;
        }
    }
    for (uint32_t m = lpr >> 1; m; m >>= 1) diff |= __shfl_xor(diff, (int)m, 64);
    const bool bad = diff && o == 0 && row < n;
    uint64_t sum[1] = {bad ? 1ull : 0ull}, mn[1] = {bad ? (row0 + row) * 2 + file : VF_NONE};
    vf_block_commit(sum, mn, cnt, {VF_C_ROWS}, {VF_C_FIRST_ROW});
}

// keys of one side's items: key[i], VF_LPI lanes an item
static __global__ void __launch_bounds__(VF_TPB) k_vf_hash(VfSide s, uint32_t F, uint32_t L, uint32_t nwords, uint64_t salt, uint64_t mask,
                                                          uint64_t *__restrict__ key) {
    const uint64_t t = (uint64_t)blockIdx.x * VF_TPB + threadIdx.x;
    const uint64_t item = t / VF_LPI;
    const uint32_t lane = (uint32_t)(t % VF_LPI);
    uint64_t acc = 0;
    if (item < s.n)
        for (uint32_t j = lane; j < nwords; j += VF_LPI) acc += vf_fmix64(vf_word(s, F, L, item, j) + (uint64_t)(j + 1) * VF_K);
    for (int m = VF_LPI >> 1; m; m >>= 1) acc += vf_shfl_xor(acc, m);
    if (item < s.n && lane == 0) key[item] = vf_fmix64(salt + acc) & mask;
}

// the values of the union: the item's index, the decoded side with bit 63
static __global__ void __launch_bounds__(VF_TPB) k_vf_vals(uint64_t n_s, uint64_t M, uint64_t *__restrict__ val) {
    const uint64_t i = (uint64_t)blockIdx.x * VF_TPB + threadIdx.x;
    if (i < M) val[i] = i < n_s ? i : ((i - n_s) | VF_SIDE_BIT);
}

struct XfVfHead {
    const uint64_t *k;
    __device__ uint64_t operator()(uint64_t i) const { return (i == 0 || k[i] != k[i - 1]) ? 1u : 0u; }
};
struct XfVfSide {
    const uint64_t *v;
    __device__ uint64_t operator()(uint64_t i) const { return v[i] >> 63; }
};

// head_pos[r] = the rank at which run r starts; head_pos[runs] = M.  run_no is the inclusive scan of the head flags
static __global__ void __launch_bounds__(VF_TPB) k_vf_head_pos(const uint64_t *__restrict__ ks, const uint64_t *__restrict__ run_no, uint64_t M,
                                                              uint64_t *__restrict__ head_pos) {
    const uint64_t i = (uint64_t)blockIdx.x * VF_TPB + threadIdx.x;
    if (i >= M) return;
    if (i == 0 || ks[i] != ks[i - 1]) head_pos[run_no[i] - 1] = i;
    if (i == M - 1) head_pos[run_no[i]] = M;
}

// every rank of the sorted union, VF_LPI lanes a rank.  In run [a, b) with cS source items (they come first, in index order)
// and cD decoded ones, offset o of one side pairs with offset o of the other; what has no partner is unmatched; a source
// item's lanes compare its pair
static __global__ void __launch_bounds__(VF_TPB) k_vf_confirm(VfSide S, VfSide D, uint32_t F, uint32_t L, uint32_t nwords, const uint64_t *__restrict__ vs,
                                                             const uint64_t *__restrict__ run_no, const uint64_t *__restrict__ head_pos,
                                                             const uint64_t *__restrict__ side_cum, uint64_t M, unsigned long long *cnt) {
    const uint64_t t = (uint64_t)blockIdx.x * VF_TPB + threadIdx.x;
    const uint64_t i = t / VF_LPI;
    const uint32_t lane = (uint32_t)(t % VF_LPI);
    uint64_t first_s = VF_NONE, first_d = VF_NONE, is = 0, id = 0;
    bool pair = false;
    if (i < M) {
        const uint64_t v = vs[i], r = run_no[i] - 1, a = head_pos[r], b = head_pos[r + 1];
        const uint64_t cD = side_cum[b] - side_cum[a], cS = (b - a) - cD;
        if (!(v & VF_SIDE_BIT)) {
            const uint64_t o = i - a;
            if (o >= cD) first_s = v;
            else {
                pair = true;
                is = v;
                id = vs[a + cS + o] & ~VF_SIDE_BIT;
            }
        } else if (i - a - cS >= cS) {
            first_d = v & ~VF_SIDE_BIT;
        }
    }
    uint32_t diff = 0;
    if (pair)
        for (uint32_t j = lane; j < nwords; j += VF_LPI) diff |= vf_word(S, F, L, is, j) != vf_word(D, F, L, id, j) ? 1u : 0u;
    for (int m = VF_LPI >> 1; m; m >>= 1) diff |= __shfl_xor(diff, m, 64);
    const bool lead = lane == 0;
    uint64_t sum[4] = {lead && pair && !diff ? 1ull : 0ull, lead && pair && diff ? 1ull : 0ull, lead && first_s != VF_NONE ? 1ull : 0ull,
                       lead && first_d != VF_NONE ? 1ull : 0ull};
    uint64_t mn[2] = {lead ? first_s : VF_NONE, lead ? first_d : VF_NONE};
    vf_block_commit(sum, mn, cnt, {VF_C_MATCHED, VF_C_UNDECIDED, VF_C_S_UNM, VF_C_D_UNM}, {VF_C_FIRST_S, VF_C_FIRST_D});
}

// rows of file f out of records that lie interleaved (record i: file i % F, row i / F): dst row r = src record r * F + f
static __global__ void __launch_bounds__(VF_TPB) k_vf_take_file(const uint8_t *__restrict__ src, uint32_t F, uint32_t f, uint32_t L, uint64_t rows,
                                                               uint8_t *__restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * VF_TPB + threadIdx.x;
    if (i >= rows * L) return;
    const uint64_t r = i / L;
    dst[i] = src[(r * F + f) * L + (i - r * L)];
}

// ------------------------------------------------------------------------------------------------ host side
static DevBufList vf_bufs(pgrc_verify *v) {
    return {&v->src_chunk[0], &v->src_chunk[1], &v->dec_chunk[0], &v->dec_chunk[1], &v->counters, &v->store[0], &v->store[1], &v->dec_rows[0], &v->dec_rows[1],
            &v->key[0], &v->key[1], &v->val[0], &v->val[1], &v->run_no, &v->head_pos, &v->side_cum};
}

static int vf_alloc(pgrc_verify *v, DevBuf &b, uint64_t bytes) {
    const int e = pgrc_buf_unpooled(v, b, bytes);
    if (!e) return PGRC_OK;
    (void)hipGetLastError();        // a refused allocation leaves the handle usable: the next launch check must not see it
    return vf_fail(v, e, v->err);
}

int pgrc_vf_open(int32_t device, uint32_t item_bytes, pgrc_verify **out) {
    *out = nullptr;
    pgrc_verify *v = new pgrc_verify();
    std::string why;
    int e = pgrc_stage_open(v, device, &why);
    if (e) {
        g_vf_begin_err = "verify: " + why;
        delete v;
        return e;
    }
    PgrcDeviceScope scope(v->device);
    for (int k = 0; k < 2 && !e; k++)
        if (hipEventCreate(&v->ev_cmp0[k]) != hipSuccess || hipEventCreate(&v->ev_cmp[k]) != hipSuccess) e = PGRC_E_DEVICE;
    if (!e) e = v->ev.ensure(v);
    if (!e) e = pgrc_buf_unpooled(v, v->counters, 8 * sizeof(unsigned long long));
    if (!e) {
        hipLaunchKernelGGL(k_vf_init_counts, dim3(1), dim3(64), 0, v->stream, (unsigned long long *)v->counters.p);
        if (hipGetLastError() != hipSuccess) e = PGRC_E_DEVICE;
    }
    if (e) {
        g_vf_begin_err = "verify: " + (v->err.empty() ? std::string("HIP event creation failed") : v->err);
        (void)hipGetLastError();
        pgrc_verify_end(v);
        return e;
    }
    v->kind = PGRC_VERIFY_MULTISET;
    v->F = 1;
    v->L = item_bytes;
    v->t_begin = std::chrono::steady_clock::now();
    *out = v;
    return PGRC_OK;
}

void pgrc_vf_mask_next_begin(uint32_t bits) { g_vf_next_bits.store(bits); }

int pgrc_vf_key_buffers(pgrc_verify *v, uint64_t n) {
    int e;
    for (int k = 0; k < 2; k++)
        if ((e = vf_alloc(v, v->key[k], n * 8)) || (e = vf_alloc(v, v->val[k], n * 8))) return e;
    if ((e = vf_alloc(v, v->run_no, n * 8)) || (e = vf_alloc(v, v->head_pos, (n + 1) * 8)) || (e = vf_alloc(v, v->side_cum, (n + 1) * 8))) return e;
    return PGRC_OK;
}

static int vf_read_counts(pgrc_verify *v, VfCounts *out) {
    unsigned long long h[8];
    HIP_TRY(v, hipMemcpyAsync(h, v->counters.p, sizeof h, hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(v, hipStreamSynchronize(v->stream));
    *out = VfCounts{h[VF_C_MATCHED], h[VF_C_UNDECIDED], h[VF_C_S_UNM], h[VF_C_D_UNM], h[VF_C_FIRST_S], h[VF_C_FIRST_D]};
    return PGRC_OK;
}

int pgrc_vf_match_keys(pgrc_verify *v, const VfSide &s, const VfSide &d, VfCounts *out) {
    const uint64_t M = s.n + d.n;
    *out = VfCounts{0, 0, 0, 0, VF_NONE, VF_NONE};
    if (!M) return PGRC_OK;
    if (M >= 0xFFFFF000ull) return vf_fail(v, PGRC_E_PARAM, "more items on both sides together than the union sort takes");
    uint32_t bits = 0;
    while (bits < 64 && (v->key_mask >> bits)) bits++;
    int e;
    HIP_TRY(v, v->ev.record(1, v->stream));
    hipLaunchKernelGGL(k_vf_vals, dim3(dec_grid(M, VF_TPB)), dim3(VF_TPB), 0, v->stream, s.n, M, (uint64_t *)v->val[0].p);
    HIP_TRY(v, hipGetLastError());
    uint64_t *ks = nullptr, *vs = nullptr;
    if ((e = pgrc_radix_sort_pairs_u64(v, (uint64_t *)v->key[0].p, (uint64_t *)v->key[1].p, (uint64_t *)v->val[0].p, (uint64_t *)v->val[1].p, M, 0, bits, v->sort_scratch,
                                       &ks, &vs)))
        return vf_fail(v, e, v->err);
    HIP_TRY(v, v->ev.record(2, v->stream));
    uint64_t *run_no = (uint64_t *)v->run_no.p, *head_pos = (uint64_t *)v->head_pos.p, *side_cum = (uint64_t *)v->side_cum.p;
    if ((e = dec_scan<true>(v, XfVfHead{ks}, M, 0, run_no)) || (e = dec_scan<false>(v, XfVfSide{vs}, M, 0, side_cum))) return e;
    hipLaunchKernelGGL(k_vf_head_pos, dim3(dec_grid(M, VF_TPB)), dim3(VF_TPB), 0, v->stream, (const uint64_t *)ks, (const uint64_t *)run_no, M, head_pos);
    HIP_TRY(v, hipGetLastError());
    HIP_TRY(v, v->ev.record(3, v->stream));
    hipLaunchKernelGGL(k_vf_init_counts, dim3(1), dim3(64), 0, v->stream, (unsigned long long *)v->counters.p);
    const uint32_t nwords = (v->F * v->L + 7) / 8;
    hipLaunchKernelGGL(k_vf_confirm, dim3(dec_grid(M * VF_LPI, VF_TPB)), dim3(VF_TPB), 0, v->stream, s, d, v->F, v->L, nwords, (const uint64_t *)vs,
                       (const uint64_t *)run_no, (const uint64_t *)head_pos, (const uint64_t *)side_cum, M, (unsigned long long *)v->counters.p);
    HIP_TRY(v, hipGetLastError());
    HIP_TRY(v, v->ev.record(4, v->stream));
    if ((e = vf_read_counts(v, out))) return e;
    v->tm.ms_sort_device += v->ev.ms(1, 2);
    v->tm.ms_scan_device += v->ev.ms(2, 3);
    v->tm.ms_confirm_device += v->ev.ms(3, 4);
    return PGRC_OK;
}

static int vf_hash_side(pgrc_verify *v, const VfSide &s, uint32_t salt, uint64_t *key) {
    if (!s.n) return PGRC_OK;
    const uint32_t nwords = (v->F * v->L + 7) / 8;
    hipLaunchKernelGGL(k_vf_hash, dim3(dec_grid(s.n * VF_LPI, VF_TPB)), dim3(VF_TPB), 0, v->stream, s, v->F, v->L, nwords, (uint64_t)salt * VF_SALT_STEP, v->key_mask, key);
    HIP_TRY(v, hipGetLastError());
    return PGRC_OK;
}

// chunk k's buffers are free again: its compare has read them
static int vf_wait_chunk(pgrc_verify *v, int k) {
    if (!v->cmp_pending[k]) return PGRC_OK;
    HIP_TRY(v, hipEventSynchronize(v->ev_cmp[k]));
    v->tm.ms_compare_device += dec_elapsed(v->ev_cmp0[k], v->ev_cmp[k]);
    v->cmp_pending[k] = false;
    return PGRC_OK;
}

static uint64_t vf_chunk_rows(const pgrc_verify *v) { return std::max<uint64_t>(16, (VF_CHUNK_BYTES / (v->L + 1)) & ~15ull); }

// IN_ORDER: n source rows of file f (row r at sp + r * sstride, device memory, queued on the handle's stream), at most one
// chunk, follow the file's rows so far; the job's rows of the range are made into chunk k's buffer and compared
static int vf_compare_rows(pgrc_verify *v, uint32_t f, const uint8_t *sp, uint64_t sstride, uint64_t n, int k) {
    const uint64_t first = v->n_src[f];
    const uint64_t m = first < v->n_dec[f] ? std::min(n, v->n_dec[f] - first) : 0;
    int e;
    if (m) {
        const uint32_t L = v->L;
        if ((e = vf_wait_chunk(v, k)) || (e = vf_alloc(v, v->dec_chunk[k], m * (L + 1) + VF_PAD))) return e;
        if ((e = pgrc_decode_rows_device(v->job, f, first, m, v->dec_chunk[k].p))) return vf_fail(v, e, "the job's rows: " + v->job->err);
        v->tm.ms_rows_device += v->job->tm.ms_rows_device;
        uint32_t lpr = 1;
        while (lpr * 16 < L) lpr <<= 1;
        HIP_TRY(v, hipEventRecord(v->ev_cmp0[k], v->stream));
        hipLaunchKernelGGL(k_vf_compare, dim3(dec_grid(m * lpr, VF_TPB)), dim3(VF_TPB), 0, v->stream, sp, sstride, (const uint8_t *)v->dec_chunk[k].p, L, m, first, f, lpr,
                           (unsigned long long *)v->counters.p);
        HIP_TRY(v, hipGetLastError());
        HIP_TRY(v, hipEventRecord(v->ev_cmp[k], v->stream));
        v->cmp_pending[k] = true;
    }
    v->n_src[f] += n;
    return PGRC_OK;
}

// MULTISET: room for `rows` rows of file f in its store; what it holds stays
static int vf_store_reserve(pgrc_verify *v, uint32_t f, uint64_t rows) {
    const uint64_t need = rows * v->L + VF_PAD;
    DevBuf &b = v->store[f];
    if (b.p && b.bytes >= need) return PGRC_OK;
    // the job's row count first: a source as long as the job never moves; anything longer doubles
    const uint64_t want = std::max<uint64_t>({need, (uint64_t)b.bytes * 2, v->n_dec[f] * v->L + VF_PAD});
    DevBuf nb;
    int e;
    if ((e = vf_alloc(v, nb, want))) return e;
    if (v->n_src[f]) HIP_TRY(v, hipMemcpyAsync(nb.p, b.p, v->n_src[f] * v->L, hipMemcpyDeviceToDevice, v->stream));
    HIP_TRY(v, hipStreamSynchronize(v->stream));
    dec_free(b);
    b = nb;
    return PGRC_OK;
}

static int vf_add_checks(pgrc_verify *v, const char *who) {
    if (v->finished) return vf_fail(v, PGRC_E_STATE, std::string(who) + " after finish");
    if (!v->job) return vf_fail(v, PGRC_E_STATE, std::string(who) + " on a handle without a job");
    return PGRC_OK;
}

extern "C" {

const char *pgrc_verify_last_error(const pgrc_verify *v) { return v ? v->err.c_str() : g_vf_begin_err.c_str(); }

int pgrc_verify_begin(pgrc_decode_ctx *job, int32_t kind, pgrc_verify **out) {
    if (!out) return PGRC_E_PARAM;
    *out = nullptr;
    if (!job) { g_vf_begin_err = "verify: job is NULL"; return PGRC_E_PARAM; }
    if (kind < PGRC_VERIFY_AUTO || kind > PGRC_VERIFY_MULTISET) { g_vf_begin_err = "verify: unknown kind"; return PGRC_E_PARAM; }
    if (!job->have_order) { g_vf_begin_err = "verify: the job has no order (pgrc_decode_set_order)"; return PGRC_E_STATE; }
    const int32_t mode = job->ord.mode;
    const uint32_t F = mode == PGRC_DECODE_SE ? 1u : mode == PGRC_DECODE_PE ? 2u : (job->ord.paired ? 2u : 1u);
    uint64_t nd[2] = {0, 0};
    for (uint32_t f = 0; f < F; f++)
        if (int e = pgrc_decode_row_count(job, f, &nd[f])) { g_vf_begin_err = "verify: " + job->err; return e; }
    if (kind == PGRC_VERIFY_AUTO) kind = mode == PGRC_DECODE_ORD ? PGRC_VERIFY_IN_ORDER : PGRC_VERIFY_MULTISET;
    if (kind == PGRC_VERIFY_MULTISET && std::min(nd[0], nd[F - 1]) > PGRC_VERIFY_MAX_ITEMS) {
        g_vf_begin_err = "verify: the job has more than 0x7FFFF800 items: the MULTISET kind takes no more (the union sort's record limit)";
        return PGRC_E_PARAM;
    }
    pgrc_verify *v = nullptr;
    if (int e = pgrc_vf_open(job->device, job->L, &v)) return e;
    v->job = job;
    v->kind = kind;
    v->F = F;
    v->n_dec[0] = nd[0];
    v->n_dec[1] = nd[1];
    const uint32_t bits = g_vf_next_bits.exchange(0);
    if (bits && bits < 64) v->key_mask = (1ull << bits) - 1;
    *out = v;
    return PGRC_OK;
}

void pgrc_verify_end(pgrc_verify *v) {
    if (!v) return;
    {
        PgrcDeviceScope scope(v->device);
        if (v->stream) (void)hipStreamSynchronize(v->stream);
        dec_free_all(vf_bufs(v));
        pgrc_buf_free(v->sort_scratch);
        for (hipEvent_t ev : {v->ev_cmp0[0], v->ev_cmp0[1], v->ev_cmp[0], v->ev_cmp[1]})
            if (ev) (void)hipEventDestroy(ev);
        v->ev.release();
    }
    if (v->divider) pgrc_divider_destroy(v->divider);
    pgrc_stage_close(v);
    delete v;
}

int pgrc_verify_add_rows(pgrc_verify *v, uint32_t file, const char *rows, uint64_t n) {
    if (!v) return PGRC_E_PARAM;
    int e;
    if ((e = vf_add_checks(v, "add_rows"))) return e;
    if (file >= v->F) return vf_fail(v, PGRC_E_PARAM, "file " + std::to_string(file) + " of a job of " + std::to_string(v->F));
    if (n && !rows) return vf_fail(v, PGRC_E_PARAM, "rows is NULL");
    if (v->kind == PGRC_VERIFY_MULTISET && (n > PGRC_VERIFY_MAX_ITEMS || v->n_src[file] + n > PGRC_VERIFY_MAX_ITEMS))
        return vf_fail(v, PGRC_E_PARAM, "more than 0x7FFFF800 items: the MULTISET kind takes no more (the union sort's record limit)");
    if (!n) return PGRC_OK;
    PGRC_ON_DEVICE(v);
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t L = v->L;
    if (v->kind == PGRC_VERIFY_MULTISET) {
        if ((e = vf_store_reserve(v, file, v->n_src[file] + n))) return e;
        if ((e = dec_upload_host(v, (uint8_t *)v->store[file].p + v->n_src[file] * L, rows, n * L))) return e;
        HIP_TRY(v, hipStreamSynchronize(v->stream));
        v->n_src[file] += n;
    } else {
        const uint64_t crows = vf_chunk_rows(v);
        for (uint64_t o = 0; o < n; o += crows) {
            const uint64_t c = std::min(crows, n - o);
            const int k = v->turn;
            v->turn ^= 1;
            if ((e = vf_wait_chunk(v, k)) || (e = vf_alloc(v, v->src_chunk[k], c * L + VF_PAD))) return e;
            if ((e = dec_upload_host(v, v->src_chunk[k].p, rows + o * L, c * L))) return e;
            if ((e = vf_compare_rows(v, file, (const uint8_t *)v->src_chunk[k].p, L, c, k))) return e;
        }
        HIP_TRY(v, hipStreamSynchronize(v->stream));       // the caller's rows have been read
    }
    v->tm.bytes_up += n * L;
    v->tm.ms_upload += dec_ms_since(t0);
    return PGRC_OK;
}

}   // extern "C"
// source text of any format: the divider parses it (pgrc_divider_run_text; PGRC_READS_FASTQ is pgrc_divider_run_fastq), the rows
// are taken where it leaves them
int pgrc_vf_add_text(pgrc_verify *v, const char *who, int32_t format, const char *text, uint64_t bytes, const char *pair_text, uint64_t pair_bytes,
                     int32_t final_piece, uint64_t *consumed, uint64_t *pair_consumed, uint64_t *n_records) {
    if (!v) return PGRC_E_PARAM;
    int e;
    const std::string pre = std::string(who) + ": ";
    if ((e = vf_add_checks(v, who))) return e;
    if (!consumed || !n_records || (bytes && !text) || (pair_bytes && !pair_text) || (pair_text && !pair_consumed))
        return vf_fail(v, PGRC_E_PARAM, pre + "a NULL argument");
    if (pair_text && v->F == 1) return vf_fail(v, PGRC_E_PARAM, pre + "pair_text on a job of one file");
    if (!pair_text && v->F == 2) return vf_fail(v, PGRC_E_PARAM, pre + "a job of two files needs pair_text");
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t L = v->L, F = v->F;
    if (!v->divider) {
        pgrc_divide_params p{};
        p.read_len = L;
        p.error_limit = 1;          // no quality division: the quality lines are not looked at
        p.device = v->device;
        if ((e = pgrc_divider_create(&p, &v->divider))) return vf_fail(v, e, pre + pgrc_divider_last_error(nullptr));
    }
    pgrc_divided_reads dr;
    uint64_t n = 0;
    if ((e = pgrc_divider_run_text(v->divider, format, text, bytes, pair_text, pair_bytes, 0, final_piece, consumed, pair_consumed, &n, &dr))) {
        *consumed = 0;
        *n_records = 0;
        if (pair_consumed) *pair_consumed = 0;
        return vf_fail(v, e, pre + pgrc_divider_last_error(v->divider));
    }
    const uint8_t *d_reads = nullptr;
    uint64_t n_last = 0;
    pgrc_divider_last_reads_device(v->divider, &d_reads, &n_last);
    const uint64_t cnt[2] = {F == 2 ? (n + 1) / 2 : n, F == 2 ? n / 2 : 0};
    if (v->kind == PGRC_VERIFY_MULTISET && (v->n_src[0] + cnt[0] > PGRC_VERIFY_MAX_ITEMS || v->n_src[1] + cnt[1] > PGRC_VERIFY_MAX_ITEMS)) {
        *consumed = 0;
        *n_records = 0;
        if (pair_consumed) *pair_consumed = 0;
        return vf_fail(v, PGRC_E_PARAM, "more than 0x7FFFF800 items: the MULTISET kind takes no more (the union sort's record limit)");
    }
    *n_records = n;
    if (n) {
        PGRC_ON_DEVICE(v);
        if (n_last != n || !d_reads) return vf_fail(v, PGRC_E_DEVICE, pre + "internal: the divider's rows are not those of this run");
        float ms[3] = {0, 0, 0};
        (void)pgrc_divider_last_ms(v->divider, ms);
        v->tm.ms_fastq_parse_device += ms[0];
        v->tm.ms_fastq_pack_device += ms[1] + ms[2];
        for (uint32_t f = 0; f < F; f++) {
            if (!cnt[f]) continue;
            if (v->kind == PGRC_VERIFY_MULTISET) {
                if ((e = vf_store_reserve(v, f, v->n_src[f] + cnt[f]))) return e;
                uint8_t *dst = (uint8_t *)v->store[f].p + v->n_src[f] * L;
                if (F == 1) HIP_TRY(v, hipMemcpyAsync(dst, d_reads, n * L, hipMemcpyDeviceToDevice, v->stream));
                else hipLaunchKernelGGL(k_vf_take_file, dim3(dec_grid(cnt[f] * L, VF_TPB)), dim3(VF_TPB), 0, v->stream, d_reads, F, f, L, cnt[f], dst);
                HIP_TRY(v, hipGetLastError());
                v->n_src[f] += cnt[f];
            } else {
                // the records are compared where they lie: row r of file f is record r * F + f
                const uint64_t crows = vf_chunk_rows(v);
                for (uint64_t o = 0; o < cnt[f]; o += crows) {
                    const int k = v->turn;
                    v->turn ^= 1;
                    if ((e = vf_compare_rows(v, f, d_reads + ((uint64_t)o * F + f) * L, (uint64_t)F * L, std::min(crows, cnt[f] - o), k))) return e;
                }
            }
        }
        HIP_TRY(v, hipStreamSynchronize(v->stream));       // the divider's next run overwrites its rows
        v->tm.bytes_up += bytes + pair_bytes;
    }
    v->tm.ms_fastq += dec_ms_since(t0);
    return PGRC_OK;
}
extern "C" {

int pgrc_verify_add_fastq(pgrc_verify *v, const char *text, uint64_t bytes, const char *pair_text, uint64_t pair_bytes, int32_t final_piece, uint64_t *consumed,
                          uint64_t *pair_consumed, uint64_t *n_records) {
    return pgrc_vf_add_text(v, "add_fastq", PGRC_READS_FASTQ, text, bytes, pair_text, pair_bytes, final_piece, consumed, pair_consumed, n_records);
}

int pgrc_verify_finish(pgrc_verify *v, pgrc_verify_result *out) {
    if (!v) return PGRC_E_PARAM;
    if (!out) return vf_fail(v, PGRC_E_PARAM, "finish: out is NULL");
    if (out->struct_size != sizeof(pgrc_verify_result)) return vf_fail(v, PGRC_E_PARAM, "finish: struct_size is not sizeof(pgrc_verify_result)");
    int e;
    if ((e = vf_add_checks(v, "finish"))) return e;
    PGRC_ON_DEVICE(v);
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t F = v->F, L = v->L;
    pgrc_verify_result r{};
    r.struct_size = sizeof r;
    r.kind = v->kind;
    for (int f = 0; f < 2; f++) { r.n_source[f] = v->n_src[f]; r.n_decoded[f] = v->n_dec[f]; }
    r.first_mismatch_file = UINT32_MAX;
    r.first_mismatch_row = r.first_source_unmatched = r.first_decoded_unmatched = VF_NONE;
    bool good = true;
    for (uint32_t f = 0; f < F; f++) good = good && v->n_src[f] == v->n_dec[f];
    if (v->kind == PGRC_VERIFY_IN_ORDER) {
        if ((e = vf_wait_chunk(v, 0)) || (e = vf_wait_chunk(v, 1))) return e;
        unsigned long long h[8];
        HIP_TRY(v, hipMemcpyAsync(h, v->counters.p, sizeof h, hipMemcpyDeviceToHost, v->stream));
        HIP_TRY(v, hipStreamSynchronize(v->stream));
        r.mismatched_rows = h[VF_C_ROWS];
        if (h[VF_C_FIRST_ROW] != VF_NONE) {
            r.first_mismatch_file = (uint32_t)(h[VF_C_FIRST_ROW] & 1);
            r.first_mismatch_row = h[VF_C_FIRST_ROW] >> 1;
        }
        good = good && !r.mismatched_rows;
    } else {
        VfSide S{}, D{};
        S.n = std::min(v->n_src[0], v->n_src[F - 1]);
        D.n = std::min(v->n_dec[0], v->n_dec[F - 1]);
        if (S.n + D.n >= 0xFFFFF000ull) return vf_fail(v, PGRC_E_PARAM, "finish: more items on both sides together than the union sort takes");
        for (uint32_t f = 0; f < F; f++) {
            if (D.n) {
                if ((e = vf_alloc(v, v->dec_rows[f], D.n * (L + 1) + VF_PAD))) return e;
                if ((e = pgrc_decode_rows_device(v->job, f, 0, D.n, v->dec_rows[f].p))) return vf_fail(v, e, "the job's rows: " + v->job->err);
                v->tm.ms_rows_device += v->job->tm.ms_rows_device;
            }
            S.p[f] = (const uint8_t *)v->store[f].p;
            S.stride[f] = L;
            D.p[f] = (const uint8_t *)v->dec_rows[f].p;
            D.stride[f] = L + 1;
        }
        VfCounts c{0, 0, 0, 0, VF_NONE, VF_NONE};
        if (S.n + D.n) {
            if ((e = pgrc_vf_key_buffers(v, S.n + D.n))) return e;
            for (uint32_t salt = 0; salt < VF_SALTS; salt++) {
                HIP_TRY(v, v->ev.record(0, v->stream));
                if ((e = vf_hash_side(v, S, salt, (uint64_t *)v->key[0].p)) || (e = vf_hash_side(v, D, salt, (uint64_t *)v->key[0].p + S.n))) return e;
                if ((e = pgrc_vf_match_keys(v, S, D, &c))) return e;
                v->tm.ms_hash_device += v->ev.ms(0, 1);
                r.salts_used = salt + 1;
                if (!c.undecided) break;
            }
        }
        r.source_unmatched = c.s_unmatched;
        r.decoded_unmatched = c.d_unmatched;
        r.undecided = c.undecided;
        r.first_source_unmatched = c.first_s;
        r.first_decoded_unmatched = c.first_d;
        good = good && !c.s_unmatched && !c.d_unmatched && !c.undecided;
    }
    r.ok = good ? 1 : 0;
    *out = r;
    v->finished = true;
    v->tm.salts_used = r.salts_used;
    uint64_t held = 0;
    for (DevBuf *b : vf_bufs(v)) held += b->bytes;
    v->tm.bytes_resident = held + v->sort_scratch.bytes;
    v->tm.ms_finish = dec_ms_since(t0);
    v->tm.ms_total = dec_ms_since(v->t_begin);
    return PGRC_OK;
}

int pgrc_verify_get_timing(pgrc_verify *v, pgrc_verify_timing *out) {
    if (!v) return PGRC_E_PARAM;
    if (!out || out->struct_size != sizeof(pgrc_verify_timing)) return vf_fail(v, PGRC_E_PARAM, "get_timing: out is NULL or its struct_size is not sizeof(pgrc_verify_timing)");
    *out = v->tm;
    out->struct_size = sizeof(pgrc_verify_timing);
    return PGRC_OK;
}

}   // extern "C"
