// decctx.h -- the decode context of include/pgrc_decode.h and the helpers its sources share: decode.hip (the reads
// rebuild), restore.hip (the restore of the matched pseudogenomes), pairpos.hip (the pair positions of the paired ORD mode)
// and pairorder.hip (the pair order of the paired non-ORD mode).
#pragma once

#include <string.h>

#include <algorithm>
#include <string>

#include "ctx.h"
#include "pgrc_decode.h"

#define DEC_TPB 256
#define DEC_TEXT_PAD 64         // zero bytes after the text: aligned 16-byte loads past a window's end stay inside
#define DEC_STAGE_BYTES (64ull << 20)

struct DecBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

struct pgrc_decode_ctx {
    uint32_t L = 0;
    int device = 0;
    hipStream_t stream = nullptr, copy_stream = nullptr;
    hipEvent_t ev_made[2]{}, ev_copied[2]{}, ev_k0[2]{}, ev_a{}, ev_b{};
    uint8_t *stage[2]{};        // pinned staging (uploads and downloads of pageable memory)
    DecBuf chunk[2];            // device chunks of rows
    DecBuf text, flag, scratch;
    uint64_t text_len = 0;
    bool have_text = false;
    struct List {
        DecBuf pos, rc, mcum, moff, msym, raw;
        uint64_t n = 0, nmis = 0;
        bool has_pos = false, has_rc = false, has_mis = false;
        uint32_t form = 0;
        char order[5];
        uint64_t text_base = 0;
    } lst[3];
    uint32_t nl = 0;
    bool have_order = false;
    pgrc_decode_order ord{};
    DecBuf rl_order, org2pos, rank;
    pgrc_decode_timing tm{};
    // pgrc_decode_set_mapped_text (restore.hip): the parts of the restored text, its scratch (kept for the next call,
    // freed with the context) and its timing
    bool have_parts = false;
    uint64_t part_len[3] = {};
    DecBuf rs_mapped, rs_marks, rs_vals, rs_ptr, rs_bsum;   // the mapped parts and streams; per-mark arrays; values; pointers; block counts
    pgrc_decode_restore_timing rtm{};
    // the pair-position coding (pairpos.hip): the uploaded input, the sort's records (and values, W = 8) in turn, per-rank
    // and per-far-pair arrays, the device-side output, scan scratch; radix.hip's sort runs on a private match-context
    // shell that borrows this context's stream (pp_mc, made on first use), with pp_sort as its scratch
    DecBuf pp_in, pp_rec[2], pp_val[2], pp_rank, pp_far, pp_out, pp_bsum;
    pgrc_match_ctx *pp_mc = nullptr;
    DevBuf pp_sort;
    hipEvent_t pp_ev[6]{};
    bool have_pp_timing = false;
    pgrc_pairpos_timing ptm{};
    // the pair-order coding (pairorder.hip): the joined orgIdx, rev, per-entry and per-pair arrays, the device-side streams,
    // scan scratch and the two error words
    DecBuf po_in, po_rev, po_ent, po_pair, po_out, po_bsum;
    hipEvent_t po_ev[11]{};
    bool have_po_timing = false;
    pgrc_pairorder_timing potm{};
    std::string err;
};

// pairpos.hip: the file-major positions of `s` as n_total u64 at d_out (device, on d->stream; synchronised on return);
// fills d->ptm but for ms_download / ms_call
int pgrc_pairpos_decode_device(pgrc_decode_ctx *d, const pgrc_pairpos_streams *s, uint64_t *d_out);
int pgrc_pairpos_check_streams(pgrc_decode_ctx *d, const pgrc_pairpos_streams *s);   // the checks that need no device (PGRC_E_PARAM)
void pgrc_pairpos_release(pgrc_decode_ctx *d);     // the buffers, events and shell above (pgrc_decode_destroy)
void pgrc_pairorder_release(pgrc_decode_ctx *d);   // pairorder.hip: its buffers and events (pgrc_decode_destroy)

#define DEC_TRY(d, expr)                                                                     \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess) {                                                             \
            (d)->err = std::string(#expr) + ": " + hipGetErrorString(e__);               \
            return pgrc_hip_code(e__);                                                       \
        }                                                                                    \
    } while (0)

static int dec_fail(pgrc_decode_ctx *d, int code, const std::string &msg) {
    d->err = msg;
    return code;
}

static int dec_buf(pgrc_decode_ctx *d, DecBuf &b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.p && b.bytes >= bytes) return PGRC_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        b.p = nullptr;
        return dec_fail(d, pgrc_hip_code(e), "hipMalloc(" + std::to_string(bytes) + "): " + hipGetErrorString(e));
    }
    b.bytes = bytes;
    return PGRC_OK;
}

static void dec_free(DecBuf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

static float dec_elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return ms;
}

static int dec_clear_err(pgrc_decode_ctx *d) {
    DEC_TRY(d, hipMemsetAsync(d->flag.p, 0, 4, d->stream));
    return PGRC_OK;
}

// host -> device through the two pinned staging buffers: the copy of one overlaps the host's fill of the other
static int dec_upload(pgrc_decode_ctx *d, void *d_dst, const void *h_src, uint64_t bytes) {
    const uint8_t *src = (const uint8_t *)h_src;
    uint8_t *dst = (uint8_t *)d_dst;
    int k = 0;
    for (uint64_t o = 0; o < bytes; o += DEC_STAGE_BYTES, k ^= 1) {
        const uint64_t c = std::min<uint64_t>(DEC_STAGE_BYTES, bytes - o);
        DEC_TRY(d, hipEventSynchronize(d->ev_copied[k]));
        memcpy(d->stage[k], src + o, c);
        DEC_TRY(d, hipMemcpyAsync(dst + o, d->stage[k], c, hipMemcpyHostToDevice, d->stream));
        DEC_TRY(d, hipEventRecord(d->ev_copied[k], d->stream));
    }
    return PGRC_OK;
}

// ------------------------------------------------------------------------------------------------ scans (u64 results)
// The three-kernel scan of export.hip's k_scan_* restated over a transform of the input: per-block sums, one block that
// scans them, per-block rescan with the carried-in prefix.
#define DS_EPT 16
#define DS_EPB (DEC_TPB * DS_EPT)

__device__ __forceinline__ uint64_t ds_block_exclusive(uint64_t v, uint64_t *smem, uint64_t *total) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint64_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t u = __shfl_up(inc, o, 64);
        if (lane >= (uint32_t)o) inc += u;
    }
    if (lane == 63) smem[wv] = inc;
    __syncthreads();
    uint64_t woff = 0, tot = 0;
    for (uint32_t k = 0; k < DEC_TPB / 64; k++) {
        const uint64_t s = smem[k];
        if (k < wv) woff += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return woff + inc - v;
}

struct XfU8 { const uint8_t *p; __device__ uint64_t operator()(uint64_t i) const { return p[i]; } };
struct XfU16 { const uint16_t *p; __device__ uint64_t operator()(uint64_t i) const { return p[i]; } };
struct XfBelow { const uint64_t *p; uint64_t lim; __device__ uint64_t operator()(uint64_t i) const { return p[i] < lim ? 1u : 0u; } };

template <typename Xf>
__global__ void __launch_bounds__(DEC_TPB) k_ds_sums(Xf xf, uint64_t n, uint64_t *bsum) {
    __shared__ uint64_t smem[DEC_TPB / 64];
    const uint64_t base = (uint64_t)blockIdx.x * DS_EPB + (uint64_t)threadIdx.x * DS_EPT;
    uint64_t s = 0;
    for (int k = 0; k < DS_EPT; k++)
        if (base + k < n) s += xf(base + k);
    uint64_t tot;
    ds_block_exclusive(s, smem, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

static __global__ void __launch_bounds__(DEC_TPB) k_ds_bsums(uint64_t *bsum, uint64_t nb) {
    __shared__ uint64_t smem[DEC_TPB / 64];
    uint64_t run = 0;
    for (uint64_t b0 = 0; b0 < nb; b0 += DEC_TPB) {
        const uint64_t i = b0 + threadIdx.x;
        const uint64_t v = i < nb ? bsum[i] : 0;
        uint64_t tot;
        const uint64_t ex = ds_block_exclusive(v, smem, &tot);
        if (i < nb) bsum[i] = run + ex;
        run += tot;
    }
    if (threadIdx.x == 0) bsum[nb] = run;
}

// out[i] = base + (INCLUSIVE ? sum of xf(0..i) : sum of xf(0..i-1)); the exclusive form also writes out[n] = base + total
template <typename Xf, bool INCLUSIVE>
__global__ void __launch_bounds__(DEC_TPB) k_ds_write(Xf xf, uint64_t n, const uint64_t *__restrict__ bsum, uint64_t nb, uint64_t base_val,
                                                      uint64_t *__restrict__ out) {
    __shared__ uint64_t smem[DEC_TPB / 64];
    const uint64_t base = (uint64_t)blockIdx.x * DS_EPB + (uint64_t)threadIdx.x * DS_EPT;
    uint64_t v[DS_EPT], s = 0;
#pragma unroll
    for (int k = 0; k < DS_EPT; k++) {
        v[k] = (base + k < n) ? xf(base + k) : 0;
        s += v[k];
    }
    uint64_t tot;
    uint64_t acc = base_val + bsum[blockIdx.x] + ds_block_exclusive(s, smem, &tot);
#pragma unroll
    for (int k = 0; k < DS_EPT; k++) {
        if (base + k < n) out[base + k] = INCLUSIVE ? acc + v[k] : acc;
        acc += v[k];
    }
    if (!INCLUSIVE && blockIdx.x == 0 && threadIdx.x == 0) out[n] = base_val + bsum[nb];
}

static __global__ void k_ds_set(uint64_t *out, uint64_t v) { *out = v; }

template <bool INCLUSIVE, typename Xf>
static int dec_scan(pgrc_decode_ctx *d, Xf xf, uint64_t n, uint64_t base_val, uint64_t *d_out) {
    const uint64_t nb = (n + DS_EPB - 1) / DS_EPB;
    int e;
    if ((e = dec_buf(d, d->scratch, (nb + 2) * sizeof(uint64_t)))) return e;
    uint64_t *bs = (uint64_t *)d->scratch.p;
    if (!n) {
        if (!INCLUSIVE) hipLaunchKernelGGL(k_ds_set, dim3(1), dim3(1), 0, d->stream, d_out, base_val);
        DEC_TRY(d, hipGetLastError());
        return PGRC_OK;
    }
    hipLaunchKernelGGL((k_ds_sums<Xf>), dim3((uint32_t)nb), dim3(DEC_TPB), 0, d->stream, xf, n, bs);
    hipLaunchKernelGGL(k_ds_bsums, dim3(1), dim3(DEC_TPB), 0, d->stream, bs, nb);
    hipLaunchKernelGGL((k_ds_write<Xf, INCLUSIVE>), dim3((uint32_t)nb), dim3(DEC_TPB), 0, d->stream, xf, n, (const uint64_t *)bs, nb, base_val, d_out);
    DEC_TRY(d, hipGetLastError());
    return PGRC_OK;
}

// complementsLut (helper.cpp:243-262): IUPAC complements of both cases to upper case, every other byte to 0
static __device__ __forceinline__ uint8_t dec_complement(uint32_t c) {
    const uint32_t u = c & 0xDFu;   // upper case (only letters are mapped)
    if (c < 'A' || (c > 'Z' && c < 'a') || c > 'z') return 0;
    switch (u) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    case 'N': return 'N';
    case 'U': return 'A';
    case 'Y': return 'R';
    case 'R': return 'Y';
    case 'K': return 'M';
    case 'M': return 'K';
    case 'B': return 'V';
    case 'V': return 'B';
    case 'D': return 'H';
    case 'H': return 'D';
    default: return 0;
    }
}
