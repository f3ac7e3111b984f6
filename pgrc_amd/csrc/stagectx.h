// stagectx.h -- the stage handle: what every encoder and decoder stage beside the matcher needs of the device.  A stage is a
// PgrcDev (device, stream, error text) with two page-locked staging buffers, the events that guard their reuse, a flag word
// for device-side findings and a grow-only scratch for the shared scan.  The decode context (decctx.h) is one with the decoder's
// state on top; the overlap search (pgovl.hip), the read sets (rsetsctx.h), the reads list (rlistctx.h) and the verifier
// (verifyctx.h) are one with their own buffers on top; the assembly (pgasm.hip) keeps a decode context.  The list codings'
// states (codingctx.h) run on any of them.  DESIGN.md 4.22.
#pragma once

#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>

#include "ctx.h"
#include "scanops.h"

#define DEC_STAGE_BYTES (64ull << 20)

struct PgrcStage : PgrcDev {
    uint8_t *stage[2]{};        // pinned staging (uploads and downloads of pageable memory)
    hipEvent_t ev_copied[2]{};  // the last upload out of stage[k] has been read
    DevBuf flag, scratch;       // 16 bytes of error flags; the scratch of dec_scan
};

// decode.hip: the device checks, the stream, the staging buffers with their events and the flag word, all at once.  A failure
// leaves its text in *create_err and the stage closed.
int pgrc_stage_open(PgrcStage *s, int32_t device, std::string *create_err);
void pgrc_stage_close(PgrcStage *s);    // waits for the stream; safe on a stage that never opened

static inline uint64_t dec_a16(uint64_t b) { return (b + 15) & ~15ull; }
static inline uint32_t dec_grid(uint64_t n, uint32_t tpb) { return (uint32_t)((n + tpb - 1) / tpb); }

static int dec_fail(PgrcStage *d, int code, const std::string &msg) {
    d->err = msg;
    return code;
}

static int dec_clear_err(PgrcStage *d) {
    HIP_TRY(d, hipMemsetAsync(d->flag.p, 0, 4, d->stream));
    return PGRC_OK;
}

// host -> device through the two pinned staging buffers: the copy of one overlaps the host's fill of the other
static int dec_upload(PgrcStage *d, void *d_dst, const void *h_src, uint64_t bytes) {
    const uint8_t *src = (const uint8_t *)h_src;
    uint8_t *dst = (uint8_t *)d_dst;
    int k = 0;
    for (uint64_t o = 0; o < bytes; o += DEC_STAGE_BYTES, k ^= 1) {
        const uint64_t c = std::min<uint64_t>(DEC_STAGE_BYTES, bytes - o);
        HIP_TRY(d, hipEventSynchronize(d->ev_copied[k]));
        memcpy(d->stage[k], src + o, c);
        HIP_TRY(d, hipMemcpyAsync(dst + o, d->stage[k], c, hipMemcpyHostToDevice, d->stream));
        HIP_TRY(d, hipEventRecord(d->ev_copied[k], d->stream));
    }
    return PGRC_OK;
}

// the same from memory that may be page-locked: then the copy engine reads it where it is
static int dec_upload_host(PgrcStage *d, void *dst, const void *src, uint64_t bytes) {
    if (!bytes || !pgrc_host_pinned(src)) return dec_upload(d, dst, src, bytes);
    HIP_TRY(d, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, d->stream));
    return PGRC_OK;
}

// device -> host, after all that is queued on the stream; returns with the stream idle.  Page-locked memory is written where
// it is, other memory through stage[0]: an upload may still be reading that buffer, and it is queued on this same stream in
// front of the copy, so its event is all there is to wait for
static int dec_download_host(PgrcStage *d, void *h_dst, const void *d_src, uint64_t bytes) {
    if (!bytes || pgrc_host_pinned(h_dst)) {
        if (bytes) HIP_TRY(d, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(d, hipStreamSynchronize(d->stream));
        return PGRC_OK;
    }
    HIP_TRY(d, hipEventSynchronize(d->ev_copied[0]));
    for (uint64_t o = 0; o < bytes; o += DEC_STAGE_BYTES) {
        const uint64_t c = std::min<uint64_t>(DEC_STAGE_BYTES, bytes - o);
        HIP_TRY(d, hipMemcpyAsync(d->stage[0], (const uint8_t *)d_src + o, c, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(d, hipStreamSynchronize(d->stream));
        memcpy((uint8_t *)h_dst + o, d->stage[0], c);
    }
    return PGRC_OK;
}

// A result block: N parts one behind the other in one page-locked block, each at a 16-byte aligned place with 16 bytes behind it
template <int N>
struct DecBlockLayout {
    uint64_t at[N], bytes[N], total;
};
template <int N>
static DecBlockLayout<N> dec_block_layout(const uint64_t (&bytes)[N]) {
    DecBlockLayout<N> o;
    o.total = 0;
    for (int k = 0; k < N; k++) {
        o.at[k] = o.total;
        o.bytes[k] = bytes[k];
        o.total += dec_a16(bytes[k]) + 16;
    }
    return o;
}

// the block of `h.total` bytes (it may exceed the parts: room for what the host writes behind them) with every non-empty part
// copied from src[k] after all that is queued on the stream; returns with the stream idle, the block at *blk (the caller's, to
// give back with hipHostFree) and the copied bytes in *down.  A failure leaves no block.
template <int N>
static int dec_download_block(PgrcStage *d, const std::string &who, const DecBlockLayout<N> &h, const void *const (&src)[N], uint8_t **blk, uint64_t *down) {
    *blk = nullptr;
    *down = 0;
    uint8_t *b = nullptr;
    hipError_t he = hipHostMalloc((void **)&b, h.total);
    if (he != hipSuccess) {
        (void)hipGetLastError();
        return dec_fail(d, PGRC_E_ALLOC, who + ": hipHostMalloc(" + std::to_string(h.total) + ") failed");
    }
    for (int k = 0; k < N && he == hipSuccess; k++) {
        if (h.bytes[k]) he = hipMemcpyAsync(b + h.at[k], src[k], h.bytes[k], hipMemcpyDeviceToHost, d->stream);
        *down += h.bytes[k];
    }
    if (he == hipSuccess) he = hipStreamSynchronize(d->stream);
    if (he != hipSuccess) {
        (void)hipHostFree(b);
        return dec_fail(d, pgrc_hip_code(he), who + ": copy down: " + hipGetErrorString(he));
    }
    *blk = b;
    return PGRC_OK;
}

// out[i] = base_val + (INCLUSIVE ? sum of xf(0..i) : sum of xf(0..i-1)); the exclusive form also writes out[n] = base_val + total
template <bool INCLUSIVE, typename Xf>
static int dec_scan(PgrcStage *d, Xf xf, uint64_t n, uint64_t base_val, uint64_t *d_out) {
    int e;
    if ((e = pgrc_buf_unpooled(d, d->scratch, sco_scratch_elems(n) * sizeof(uint64_t)))) return e;
    HIP_TRY(d, (sco_device_scan<INCLUSIVE, true>(d->stream, xf, n, ScoPlus{}, (uint64_t)0, base_val, ScoStore<uint64_t>{d_out}, (uint64_t *)d->scratch.p)));
    return PGRC_OK;
}
