// results.hip -- result-state plumbing and mismatch extraction.
//
//   init   : DefaultReadsMatcher::initMatching, matching/ReadsMatchers.cpp:97-105, :411-415
//   hist   : matchedCountPerMismatches / matchedReadsCount (ReadsMatchers.h:35,116).  The reference
//            maintains them incrementally (:439-447); at any point they equal the histogram of
//            readMismatchesCount[], which is what this kernel computes once per run.
//   extract: AbstractReadsApproxMatcher::updateEntry :548-559 with fillEntryWithMismatches :40-51 and
//            fillEntryWithReversedMismatches :53-66; code = (val(pg)<<4)+val(read), helper.cpp:358-362.
#include "ctx.h"
#include "devutil.h"
#include "scanops.h"

__global__ void __launch_bounds__(256) k_init_results(uint64_t *pos, uint8_t *rc, uint8_t *mism, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        pos[i] = PGRC_NOT_MATCHED_POS;
        rc[i] = 0;
        mism[i] = PGRC_NOT_MATCHED_CNT;
    }
}

int pgrc_launch_init_results(pgrc_match_ctx *c) {
    if (!c->rd.n) return PGRC_OK;
    uint32_t grid = (uint32_t)((c->rd.n + 255) / 256 < 65536 ? (c->rd.n + 255) / 256 : 65536);
    hipLaunchKernelGGL(k_init_results, dim3(grid), dim3(256), 0, c->stream, (uint64_t *)c->res.d_pos.p, (uint8_t *)c->res.d_rc.p,
                       (uint8_t *)c->res.d_mism.p, c->rd.n);
    HIP_TRY(c, hipGetLastError());
    return PGRC_OK;
}

// Takes the dual kernel's packed words apart (dualkern.h, "The packed result"): a tagged pos[i] becomes the clean
// position, rc[i] and mism[i].  NOTHING is stored for a read without the tag, and rc / mism are written byte by byte, never
// as read-modify-written vectors: beside this pass the N kernel on the side stream writes other reads' bytes of the same
// lines, and in a second-phase run the untagged reads hold earlier results.
__global__ void __launch_bounds__(256) k_unpack_results(uint64_t *pos, uint8_t *rc, uint8_t *mism, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t v = pos[i];
        if ((v >> 62) == 1ull) {
            pos[i] = v & RES_PACK_POS_MASK;
            rc[i] = (uint8_t)((v >> RES_PACK_RC_SHIFT) & 1ull);
            mism[i] = (uint8_t)(v >> RES_PACK_MISM_SHIFT);
        }
    }
}

int pgrc_launch_unpack_results(pgrc_match_ctx *c, uint64_t lo, uint64_t n) {
    if (!n) return PGRC_OK;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)c->num_cus * 16u);
    hipLaunchKernelGGL(k_unpack_results, dim3(grid), dim3(256), 0, c->stream, (uint64_t *)c->res.d_pos.p + lo, (uint8_t *)c->res.d_rc.p + lo,
                       (uint8_t *)c->res.d_mism.p + lo, n);
    HIP_TRY(c, hipGetLastError());
    return PGRC_OK;
}

__global__ void __launch_bounds__(256) k_hist(const uint8_t *__restrict__ mism, uint64_t n, unsigned long long *hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    // 16 counts per thread and pass keep the LDS counters far from u32 overflow
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        atomicAdd(&h[mism[i]], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

int pgrc_launch_hist(pgrc_match_ctx *c) {
    HIP_TRY(c, hipMemsetAsync(c->res.d_hist.p, 0, 256 * sizeof(uint64_t), c->stream));
    if (c->rd.n) {
        uint32_t grid = (uint32_t)((c->rd.n + 255) / 256 < 2048 ? (c->rd.n + 255) / 256 : 2048);
        hipLaunchKernelGGL(k_hist, dim3(grid), dim3(256), 0, c->stream, (const uint8_t *)c->res.d_mism.p, c->rd.n,
                           (unsigned long long *)c->res.d_hist.p);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(c->res.hist, c->res.d_hist.p, 256 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->res.matched = c->rd.n - c->res.hist[PGRC_NOT_MATCHED_CNT];
    return PGRC_OK;
}

// ---------------------------------------------------------------- mismatch extraction

__device__ __forceinline__ uint32_t mcount(uint8_t m) { return m == PGRC_NOT_MATCHED_CNT ? 0u : (uint32_t)m; }
struct XsCount { __device__ uint32_t operator()(uint8_t m) const { return mcount(m); } };    // a read's mismatch count (255 -> 0)

struct ExtractArgs {
    const uint32_t *pg;
    const uint32_t *reads;
    uint64_t n, stride;
    const uint8_t *nflag;
    const uint32_t *nidx;
    const uint8_t *nascii;
    uint64_t nn;
    const uint64_t *pos;
    const uint8_t *rc, *mism, *revflags;
    const uint64_t *cum;
    uint8_t *codes;
    uint16_t *offsets;
    uint32_t L;
};

// value of symbol x of the ORIGINAL read: 0..3, or 4 for 'N' (byte path)
template <bool ASCII>
__device__ __forceinline__ uint32_t read_val(const ExtractArgs &a, uint64_t i, uint64_t t, uint32_t x) {
    if (ASCII) {
        const uint8_t ch = a.nascii[t * a.L + x];
        return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
    }
    return (a.reads[(uint64_t)(x >> 4) * a.stride + i] >> (2u * (x & 15u))) & 3u;
}
__device__ __forceinline__ uint32_t compl_val(uint32_t v) { return v < 4u ? 3u - v : 4u; } // N <-> N

template <bool ASCII>
__global__ void __launch_bounds__(256) k_extract(const ExtractArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t i;
    if (ASCII) {
        if (t >= a.nn) return;
        i = a.nidx[t];
    } else {
        if (t >= a.n) return;
        i = t;
        if (a.nflag && a.nflag[i]) return;
    }
    const uint32_t cnt = mcount(a.mism[i]);
    if (!cnt) return;
    const uint64_t p = a.pos[i];
    const bool rc = a.rc[i] != 0;
    const bool reversed = a.revflags ? a.revflags[i] != 0 : rc;
    uint64_t o = a.cum[i];
    const uint32_t L = a.L;
    uint32_t emitted = 0;
    for (uint32_t step = 0; step < L && emitted < cnt; step++) {
        const uint32_t x = reversed ? L - 1u - step : step;     // index into the (possibly RC'd) read / Pg window
        uint32_t rv = rc ? compl_val(read_val<ASCII>(a, i, t, L - 1u - x)) : read_val<ASCII>(a, i, t, x);
        const uint64_t g = p + x;
        uint32_t pv = (a.pg[g >> 4] >> (2u * ((uint32_t)g & 15u))) & 3u;
        if (rv != pv) {
            if (reversed) { pv = compl_val(pv); rv = compl_val(rv); }
            a.codes[o] = (uint8_t)((pv << 4) + rv);
            a.offsets[o] = (uint16_t)step; // forward: x; reversed: L-1-x
            o++;
            emitted++;
        }
    }
}

// The lists on the device: d_cum (u64[n + 1], exclusive scan of the reads' mismatch counts), d_codes / d_offs (one entry per
// mismatch), *total.  d_revflags: per-read orientation flags ON THE DEVICE (nullptr: reversed iff the read matched the RC strand).
// Everything is queued on c->stream; the call returns after the scan's total is known (one synchronisation).
int pgrc_extract_lists_device(pgrc_match_ctx *c, const uint8_t *d_revflags, bool lists, DevBuf &d_cum, DevBuf &d_codes, DevBuf &d_offs, uint64_t *total_out) {
    const uint64_t n = c->rd.n;
    DevBuf d_bsum;
    int e;
    if ((e = pgrc_buf_ensure(c, d_cum, (n + 1) * sizeof(uint64_t)))) return e;
    if ((e = pgrc_buf_ensure(c, d_bsum, sco_scratch_elems(n) * sizeof(uint64_t)))) return e;
    // d_cum = exclusive scan of the counts in u64, d_cum[n] = their total
    const hipError_t he = sco_device_scan<false, true>(c->stream, ScoLoad<uint64_t, uint8_t, XsCount>{(const uint8_t *)c->res.d_mism.p, XsCount{}}, n, ScoPlus{}, (uint64_t)0, (uint64_t)0,
                                                 ScoStore<uint64_t>{(uint64_t *)d_cum.p}, (uint64_t *)d_bsum.p);
    uint64_t total = 0;
    if (he != hipSuccess || hipMemcpyAsync(&total, (const uint64_t *)d_cum.p + n, sizeof total, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        pgrc_buf_free(d_bsum);
        c->err = "extract: scan failed";
        return PGRC_E_DEVICE;
    }
    pgrc_buf_free(d_bsum);
    *total_out = total;
    if (!total || !lists) return PGRC_OK;                   // (lists = false: only the counts' scan was asked for)
    if ((e = pgrc_buf_ensure(c, d_codes, total)) || (e = pgrc_buf_ensure(c, d_offs, total * sizeof(uint16_t)))) return e;
    ExtractArgs a;
    a.pg = (const uint32_t *)c->txt.pg2[0].p;
    a.reads = c->rd.reads2;
    a.n = n;
    a.stride = c->rd.stride;
    a.nflag = c->rd.n_nreads ? (const uint8_t *)c->rd.nread_flag.p : nullptr;
    a.nidx = (const uint32_t *)c->rd.nread_idx.p;
    a.nascii = (const uint8_t *)c->rd.nread_ascii.p;
    a.nn = c->rd.n_nreads;
    a.pos = (const uint64_t *)c->res.d_pos.p;
    a.rc = (const uint8_t *)c->res.d_rc.p;
    a.mism = (const uint8_t *)c->res.d_mism.p;
    a.revflags = d_revflags;
    a.cum = (const uint64_t *)d_cum.p;
    a.codes = (uint8_t *)d_codes.p;
    a.offsets = (uint16_t *)d_offs.p;
    a.L = c->prm.read_len;
    hipLaunchKernelGGL(k_extract<false>, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, a);
    if (c->rd.n_nreads)
        hipLaunchKernelGGL(k_extract<true>, dim3((uint32_t)((c->rd.n_nreads + 255) / 256)), dim3(256), 0, c->stream, a);
    if (hipGetLastError() != hipSuccess) { c->err = "extract: kernel failed"; return PGRC_E_DEVICE; }
    return PGRC_OK;
}

int pgrc_extract_mismatches(pgrc_match_ctx *c, const uint8_t *reversed_flags, uint64_t *cum, uint8_t *codes,
                            uint16_t *offsets) {
    const uint64_t n = c->rd.n;
    DevBuf d_cum, d_codes, d_offs, d_flags;
    int e;
    auto cleanup = [&]() { pgrc_buf_free(d_cum); pgrc_buf_free(d_codes); pgrc_buf_free(d_offs); pgrc_buf_free(d_flags); };
    if (reversed_flags && codes && offsets) {
        if ((e = pgrc_buf_ensure(c, d_flags, n ? n : 1))) { cleanup(); return e; }
        if (n && hipMemcpyAsync(d_flags.p, reversed_flags, n, hipMemcpyHostToDevice, c->stream) != hipSuccess) { cleanup(); return PGRC_E_DEVICE; }
    }
    uint64_t total = 0;
    const bool lists = codes && offsets;
    if ((e = pgrc_extract_lists_device(c, (reversed_flags && lists) ? (const uint8_t *)d_flags.p : nullptr, lists, d_cum, d_codes, d_offs, &total))) { cleanup(); return e; }
    bool ok = hipMemcpyAsync(cum, d_cum.p, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    if (ok && lists && total)
        ok = hipMemcpyAsync(codes, d_codes.p, total, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
             hipMemcpyAsync(offsets, d_offs.p, total * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
    cleanup();
    if (!ok) { c->err = "extract: copy failed"; return PGRC_E_DEVICE; }
    return PGRC_OK;
}
