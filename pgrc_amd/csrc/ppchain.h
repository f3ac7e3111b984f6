// ppchain.h -- the encoder's far-pair chain that the two pair codings share: pairpos.hip (compressReadsPgPositions, positions
// of W bytes and int16 deltas) and pairorder.hip (compressReadsOrder, reads-list offsets in uint32 and int8 deltas).  In both
// a far pair is a delta pair when rel - refPrev fits the delta type D, and refPrev before far pair k is rel[k-1] (state A: k-1
// was a delta pair; C: a full pair that set it; the start is C with rel[-1] = 0) or rel[k-2] (state B: k-1 was a full pair that
// kept it).  Pair k maps A -> (delta ? A : B), B -> (delta' ? A : C), C -> (delta ? A : C), delta judged against rel[k-1] and
// delta' against rel[k-2]: a map of {A, B, C} in 6 bits.  scanops.h's scan with PpCompose gives every far pair the map of all
// pairs before it, hence its state, its kind and its delta.
#pragma once

#include <chrono>
#include <limits>

#include "decctx.h"
#include "scanops.h"

#define PP_TPB 256

static uint32_t pp_grid(uint64_t n) { return std::max(1u, dec_grid(n, PP_TPB)); }      // (one block for nothing, too)

// states of the chain: what the far pair before was
#define PP_S_A 0u           // a delta pair: refPrev = its rel
#define PP_S_B 1u           // a full pair that kept refPrev = the rel of the pair before it
#define PP_S_C 2u           // a full pair that set refPrev = its rel (and the start, with rel 0)
#define PP_MAP_IDENT (PP_S_A | PP_S_B << 2 | PP_S_C << 4)

// x: a difference of two rel values in 64 bits (wrapped); D: the delta stream's element type
template <typename D>
__device__ __forceinline__ bool pp_fits(uint64_t x) {
    return (int64_t)x >= (int64_t)std::numeric_limits<D>::min() && (int64_t)x <= (int64_t)std::numeric_limits<D>::max();
}

struct PpCompose {          // first a, then b
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const {
        uint32_t r = 0;
#pragma unroll
        for (uint32_t s = 0; s < 3; s++) r |= ((b >> (2u * ((a >> (2u * s)) & 3u))) & 3u) << (2u * s);
        return r;
    }
};

// R: the element type of rel in far order (uint64_t or uint32_t)
template <typename D, typename R>
__global__ void __launch_bounds__(PP_TPB) k_pp_enc_maps(uint64_t nf, const R *__restrict__ far_rel, uint8_t *__restrict__ map) {
    const uint64_t k = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (k >= nf) return;
    const uint64_t r0 = far_rel[k], r1 = k >= 1 ? far_rel[k - 1] : 0, r2 = k >= 2 ? far_rel[k - 2] : 0;
    const bool d1 = pp_fits<D>(r0 - r1), d2 = pp_fits<D>(r0 - r2);
    map[k] = (uint8_t)((d1 ? PP_S_A : PP_S_B) | (d2 ? PP_S_A : PP_S_C) << 2 | (d1 ? PP_S_A : PP_S_C) << 4);
}

// pre[k]: the composed map of the far pairs before k; the chain starts in C
template <typename D, typename R>
__global__ void __launch_bounds__(PP_TPB) k_pp_enc_kinds(uint64_t nf, const R *__restrict__ far_rel, const uint32_t *__restrict__ pre,
                                                         uint8_t *__restrict__ del_flag, D *__restrict__ dval) {
    const uint64_t k = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (k >= nf) return;
    const uint32_t st = (pre[k] >> 4) & 3u;
    const uint64_t ref = st == PP_S_B ? (k >= 2 ? far_rel[k - 2] : 0) : (k >= 1 ? far_rel[k - 1] : 0);
    const uint64_t dl = (uint64_t)far_rel[k] - ref;
    del_flag[k] = pp_fits<D>(dl) ? 1 : 0;
    dval[k] = (D)dl;
}

// The decoders' refPrev: every far pair is ADD d (delta), SET rel (a full pair that sets it) or ADD 0 (a full pair that keeps it).
// The segmented sum: scanops.h's scan over (value, set) with (a, b) -> b.set ? b : (a.v + b.v, a.set)
struct __attribute__((packed, aligned(4))) PpSeg {      // 12 bytes: three words to shuffle
    int64_t v;
    uint32_t set;
};
__device__ __forceinline__ PpSeg pp_seg_op(PpSeg a, PpSeg b) { return b.set ? b : PpSeg{a.v + b.v, a.set}; }
struct PpSegOp { __device__ PpSeg operator()(PpSeg a, PpSeg b) const { return pp_seg_op(a, b); } };
