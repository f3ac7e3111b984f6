// pairpos.hip -- the pair-position coding of the order-preserving paired mode on the device, both directions
// (include/pgrc_decode.h, "The pair-position coding"; SeparatedPseudoGenomePersistence.cpp:445-574 and :582-673).
//
// Both of the reference's functions are a stable sort of the pairs by base position and a serial loop over the ranked pairs.
// Here the rank order is radix.hip's stable sort (records base << 32 | pair for 4-byte positions, the pairs form for 8-byte
// ones, over the position bits in use), and the loop falls apart into per-pair work between prefix scans:
//   flags -> stream indexes        scanops.h over the flag bytes (how many near / delta pairs precede a pair)
//   decoder, refPrev               every far pair is ADD d (delta), SET |mate - base| (full after a full, or the first far
//                                  pair) or KEEP (full after a delta): a segmented inclusive sum in int64 (scanops.h), run   
//                                  over ALL ranked pairs with the near ones as ADD 0, so no far-to-rank map is needed
//   encoder, refPrev               before far pair k it is rel[k-1] (state A: k-1 was a delta pair; C: a full pair that set
//                                  it; the start is C with rel[-1] = 0) or rel[k-2] (state B: k-1 was a full pair that kept
//                                  it).  Pair k maps A -> (delta ? A : B), B -> (delta' ? A : C), C -> (delta ? A : C), delta
//                                  judged against rel[k-1] and delta' against rel[k-2]: a map of {A, B, C} in 6 bits from three
//                                  neighbouring values.  Maps compose associatively: scanops.h's scan with PpCompose gives
//                                  every far pair the map of all pairs before it, hence its state, its kind and its int16.
// Integer work bound by HBM streams and gathers; no atomics, no library kernel.
#include "ppchain.h"
#include "rlistctx.h"

#define PP_MAX_PAIRS 0xFFFFF000ull     // rx_sort's record limit

// ------------------------------------------------------------------------------------------------ records, rank entries
struct PpBaseOrg {          // encoder: the interleaved array; the mate's position goes into the range check
    const uint64_t *org;
    __device__ uint64_t base(uint64_t p) const { return org[2 * p]; }
    __device__ uint64_t other(uint64_t p) const { return org[2 * p + 1]; }
};
template <typename T>
struct PpBaseStream {       // decoder: basePairPos
    const T *b;
    __device__ uint64_t base(uint64_t p) const { return b[p]; }
    __device__ uint64_t other(uint64_t) const { return 0; }
};

#define PP_OR_BLOCKS 1024
// W8: keys = positions, values = pair numbers; else records position << 32 | pair.  bor[2b], bor[2b+1]: the block's OR of the
// base positions / of everything
template <bool W8, typename Ld>
__global__ void __launch_bounds__(PP_TPB) k_pp_records(Ld ld, uint64_t P, uint64_t *__restrict__ rec, uint64_t *__restrict__ val, uint64_t *__restrict__ bor) {
    __shared__ uint64_t sm[2][PP_TPB / 64];
    uint64_t ob = 0, oa = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x; p < P; p += (uint64_t)gridDim.x * PP_TPB) {
        const uint64_t b = ld.base(p);
        ob |= b;
        oa |= ld.other(p);
        if (W8) {
            rec[p] = b;
            val[p] = p;
        } else {
            rec[p] = b << 32 | p;
        }
    }
    oa |= ob;
    for (int o = 32; o > 0; o >>= 1) {
        ob |= __shfl_xor(ob, o, 64);
        oa |= __shfl_xor(oa, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sm[0][threadIdx.x >> 6] = ob;
        sm[1][threadIdx.x >> 6] = oa;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint64_t r = 0;
        for (int k = 0; k < PP_TPB / 64; k++) r |= sm[threadIdx.x][k];
        bor[2 * blockIdx.x + threadIdx.x] = r;
    }
}

static __global__ void k_pp_or_final(const uint64_t *__restrict__ bor, uint32_t nb, uint64_t *__restrict__ out) {
    if (threadIdx.x < 2) {
        uint64_t r = 0;
        for (uint32_t k = 0; k < nb; k++) r |= bor[2 * k + threadIdx.x];
        out[threadIdx.x] = r;
    }
}

// ranked pair i of the sorted records (a = records, or keys with b = values)
template <bool W8>
__device__ __forceinline__ void pp_entry(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b, uint64_t i, uint64_t &base, uint64_t &pair) {
    const uint64_t r = a[i];
    if (W8) {
        base = r;
        pair = b[i];
    } else {
        base = r >> 32;
        pair = r & 0xFFFFFFFFull;
    }
}

struct PpIsOne { __device__ uint32_t operator()(uint32_t x) const { return x == 1u ? 1u : 0u; } };      // offsetInUint16Flag[i] == 1 (:647)
struct PpNonZero { __device__ uint32_t operator()(uint32_t x) const { return x ? 1u : 0u; } };          // if (deltaInInt16Flag[..]) (:652)

// ------------------------------------------------------------------------------------------------ decoder
#define PP_K_SET 1u         // a full pair that sets refPrev
#define PP_K_DELTA 2u       // a delta pair: its mate needs the chain
#define PP_K_BF 4u          // ... and lies after its base

struct PpDecStreams {
    const uint8_t *off16_flag, *off_bf;
    const uint16_t *off_val;
    const uint8_t *del_flag, *del_bf;
    const int16_t *del_val;
    const void *not_base;
    const uint32_t *near_inc, *del_inc;      // inclusive counts of near pairs (rank order) / delta pairs (far order)
};

// every ranked pair: the base's position; the mate of a near or full pair; the pair's entry in the chain (kind, value)
template <bool W8>
__global__ void __launch_bounds__(PP_TPB) k_pp_dec_ops(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b, uint64_t P, PpDecStreams s,
                                                       uint64_t *__restrict__ out, uint8_t *__restrict__ kind, int64_t *__restrict__ val) {
    const uint64_t i = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (i >= P) return;
    const uint64_t wmask = W8 ? ~0ull : 0xFFFFFFFFull;
    uint64_t base, pair;
    pp_entry<W8>(a, b, i, base, pair);
    out[pair] = base;
    const uint32_t ninc = s.near_inc[i];
    if (s.off16_flag[i] == 1) {
        const uint64_t j = ninc - 1u, off = s.off_val[j];
        out[P + pair] = (s.off_bf[j] == 0 ? base - off : base + off) & wmask;
        kind[i] = 0;
        return;
    }
    const uint64_t k = i - ninc;
    const uint32_t dinc = s.del_inc[k];
    if (s.del_flag[k]) {
        const uint64_t j = dinc - 1u;
        val[i] = s.del_val[j];
        kind[i] = (uint8_t)(PP_K_DELTA | (s.del_bf[j] ? PP_K_BF : 0u));
        return;
    }
    const uint64_t x = k - dinc;
    const uint64_t m = W8 ? ((const uint64_t *)s.not_base)[x] : (uint64_t)((const uint32_t *)s.not_base)[x];
    out[P + pair] = m;
    if (k > 0 && s.del_flag[k - 1]) {       // the far pair before was a delta pair: refPrev stays (:665)
        kind[i] = 0;
        return;
    }
    int64_t dl = (int64_t)(m - base);
    if (dl < 0) dl = -dl;
    val[i] = dl;
    kind[i] = (uint8_t)PP_K_SET;
}

// (the segmented sum itself -- PpSeg, PpSegOp -- is ppchain.h, shared with pairorder.hip's decoder)
struct PpChainIn {          // the chain's entry of ranked pair i: near and keeping pairs add nothing
    const uint8_t *kind;
    const int64_t *val;
    __device__ PpSeg operator()(uint64_t i) const {
        const uint32_t k = kind[i];
        if (!(k & (PP_K_SET | PP_K_DELTA))) return PpSeg{0, 0u};
        return PpSeg{val[i], k & PP_K_SET};
    }
};

// the mate of a delta pair: base +- refPrev at its place, back in pair order
template <bool W8>
struct PpDeltaSink {
    const uint64_t *a, *b;
    const uint8_t *kind;
    uint64_t P;
    uint64_t *out;
    __device__ void operator()(uint64_t i, PpSeg acc) const {          // acc: the inclusive sum at i
        const uint32_t k = kind[i];
        if (!(k & PP_K_DELTA)) return;
        const int64_t ref = acc.v;
        uint64_t base, pair;
        pp_entry<W8>(a, b, i, base, pair);
        const uint64_t m = (k & PP_K_BF) ? base + (uint64_t)ref : base - (uint64_t)ref;
        out[P + pair] = W8 ? m : (m & 0xFFFFFFFFull);
    }
};

// ------------------------------------------------------------------------------------------------ encoder
template <typename T>
__global__ void __launch_bounds__(PP_TPB) k_pp_enc_base(const uint64_t *__restrict__ org, uint64_t P, T *__restrict__ base_pos) {
    const uint64_t p = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (p < P) base_pos[p] = (T)org[2 * p];
}

// ranked pair i: rel = |mate - base|, the base-first flag, the near flag (:501-505)
template <bool W8>
__global__ void __launch_bounds__(PP_TPB) k_pp_enc_class(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b, const uint64_t *__restrict__ org, uint64_t P,
                                                         uint8_t *__restrict__ off16_flag, uint64_t *__restrict__ rel, uint8_t *__restrict__ bf) {
    const uint64_t i = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (i >= P) return;
    uint64_t base, pair;
    pp_entry<W8>(a, b, i, base, pair);
    const uint64_t mate = org[2 * pair + 1];
    const bool first = base < mate;
    const uint64_t r = first ? mate - base : base - mate;
    off16_flag[i] = r <= 65535u ? 1 : 0;
    rel[i] = r;
    bf[i] = first ? 1 : 0;
}

// near pairs -> their two streams; far pairs -> far order (rel and the rank they came from)
static __global__ void __launch_bounds__(PP_TPB) k_pp_enc_compact(uint64_t P, const uint8_t *__restrict__ off16_flag, const uint32_t *__restrict__ near_inc,
                                                                  const uint64_t *__restrict__ rel, const uint8_t *__restrict__ bf, uint8_t *__restrict__ off_bf,
                                                                  uint16_t *__restrict__ off_val, uint64_t *__restrict__ far_rel, uint32_t *__restrict__ far_rank) {
    const uint64_t i = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (i >= P) return;
    const uint32_t ninc = near_inc[i];
    if (off16_flag[i]) {
        off_bf[ninc - 1u] = bf[i];
        off_val[ninc - 1u] = (uint16_t)rel[i];
    } else {
        const uint64_t k = i - ninc;
        far_rel[k] = rel[i];
        far_rank[k] = (uint32_t)i;
    }
}

// (the chain itself -- states, maps, PpCompose, k_pp_enc_maps / k_pp_enc_kinds -- is ppchain.h, shared with pairorder.hip)
template <bool W8>
__global__ void __launch_bounds__(PP_TPB) k_pp_enc_far(uint64_t nf, const uint32_t *__restrict__ far_rank, const uint64_t *__restrict__ far_rel,
                                                       const uint8_t *__restrict__ del_flag, const uint32_t *__restrict__ del_inc, const int16_t *__restrict__ dval,
                                                       const uint8_t *__restrict__ bf, const uint64_t *__restrict__ a, const uint64_t *__restrict__ b,
                                                       uint8_t *__restrict__ del_bf, int16_t *__restrict__ del_val, void *__restrict__ not_base) {
    const uint64_t k = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (k >= nf) return;
    const uint64_t i = far_rank[k];
    const uint32_t dinc = del_inc[k];
    const bool first = bf[i] != 0;
    if (del_flag[k]) {
        del_bf[dinc - 1u] = first ? 1 : 0;
        del_val[dinc - 1u] = dval[k];
        return;
    }
    uint64_t base, pair;
    pp_entry<W8>(a, b, i, base, pair);
    const uint64_t mate = first ? base + far_rel[k] : base - far_rel[k];
    if (W8) ((uint64_t *)not_base)[k - dinc] = mate;
    else ((uint32_t *)not_base)[k - dinc] = (uint32_t)mate;
}

// ------------------------------------------------------------------------------------------------ host side
static int pp_fail(PgrcStage *d, const char *who, const std::string &msg) { return dec_fail(d, PGRC_E_PARAM, std::string(who) + ": " + msg); }

// the rank order of the P records in rec[0] (val[0]): stable by the position bits in use
static int pp_sort(PgrcStage *d, PgrcPairPos &st, bool w8, uint64_t P, uint64_t base_or, const uint64_t **a, const uint64_t **b) {
    uint32_t hb = 0;
    while (hb < 64 && (base_or >> hb)) hb++;
    uint64_t *sorted = nullptr, *vsorted = nullptr;
    int e;
    if (w8) e = pgrc_radix_sort_pairs_u64(d, (uint64_t *)st.rec[0].p, (uint64_t *)st.rec[1].p, (uint64_t *)st.val[0].p, (uint64_t *)st.val[1].p, P, 0, hb,
                                          st.sort, &sorted, &vsorted);
    else e = pgrc_radix_sort_u64(d, (uint64_t *)st.rec[0].p, (uint64_t *)st.rec[1].p, P, 32, 32 + std::min(hb, 32u), st.sort, &sorted);
    if (e) return dec_fail(d, e, "pair positions: " + d->err);
    *a = sorted;
    *b = vsorted;
    return PGRC_OK;
}

static int pp_sort_buffers(PgrcStage *d, PgrcPairPos &st, bool w8, uint64_t P) {
    int e;
    for (int k = 0; k < 2; k++) {
        if ((e = pgrc_buf_unpooled(d, st.rec[k], P * 8))) return e;
        if (w8 && (e = pgrc_buf_unpooled(d, st.val[k], P * 8))) return e;
    }
    return PGRC_OK;
}

template <bool W8>
static int pp_decode_run(PgrcStage *d, PgrcPairPos &st, const pgrc_pairpos_streams *s, uint64_t *d_out) {
    static const char *who = "pair positions (decode)";
    const uint64_t T = s->n_total, P = T / 2, W = s->pos_width;
    const uint64_t nf = s->n_delta_flag;
    const auto t0 = std::chrono::steady_clock::now();
    int e;
    if ((e = st.ev.ensure(d)) || (e = pp_sort_buffers(d, st, W8, P))) return e;
    // the streams, each at a 16-byte aligned place
    const void *hsrc[8] = {s->base_pos, s->off16_flag, s->off_base_first, s->off_value, s->delta16_flag, s->delta_base_first, s->delta_value, s->not_base_pos};
    const uint64_t nbytes[8] = {P * W, P, s->n_off16, s->n_off16 * 2, nf, s->n_delta16, s->n_delta16 * 2, s->n_not_base * W};
    uint64_t at[8], in_bytes = 0, up = 0;
    for (int k = 0; k < 8; k++) {
        at[k] = in_bytes;
        in_bytes += dec_a16(nbytes[k]) + 16;
        up += nbytes[k];
    }
    const uint64_t near_at = 0, kind_at = near_at + dec_a16(P * 4) + 16, val_at = kind_at + dec_a16(P) + 16, rank_bytes = val_at + P * 8 + 16;
    const uint64_t bsum_bytes = dec_a16(sco_scratch_elems(std::max(P, nf)) * sizeof(PpSeg)) + 2 * PP_OR_BLOCKS * 8 + 64;     // (the flag scans' u32 folds too)
    if ((e = pgrc_bufs_unpooled(d, {{&st.in, in_bytes}, {&st.rank, rank_bytes}, {&st.far, nf * 4 + 16}, {&st.bsum, bsum_bytes}}))) return e;
    uint8_t *in = (uint8_t *)st.in.p;
    for (int k = 0; k < 8; k++)
        if (nbytes[k] && (e = dec_upload(d, in + at[k], hsrc[k], nbytes[k]))) return e;
    const float ms_upload = dec_ms_since(t0);
    PpDecStreams ds;
    ds.off16_flag = in + at[1];
    ds.off_bf = in + at[2];
    ds.off_val = (const uint16_t *)(in + at[3]);
    ds.del_flag = in + at[4];
    ds.del_bf = in + at[5];
    ds.del_val = (const int16_t *)(in + at[6]);
    ds.not_base = in + at[7];
    uint32_t *near_inc = (uint32_t *)((uint8_t *)st.rank.p + near_at), *del_inc = (uint32_t *)st.far.p;
    uint8_t *kind = (uint8_t *)st.rank.p + kind_at;
    int64_t *val = (int64_t *)((uint8_t *)st.rank.p + val_at);
    ds.near_inc = near_inc;
    ds.del_inc = del_inc;
    uint64_t *bor = (uint64_t *)((uint8_t *)st.bsum.p + bsum_bytes - 2 * PP_OR_BLOCKS * 8 - 32);     // block ORs, then the two results
    uint32_t *sco_tmp = (uint32_t *)st.bsum.p;

    HIP_TRY(d, st.ev.record(0, d->stream));
    const uint32_t nor = (uint32_t)std::min<uint64_t>(pp_grid(P), PP_OR_BLOCKS);
    if (W8) hipLaunchKernelGGL((k_pp_records<true, PpBaseStream<uint64_t>>), dim3(nor), dim3(PP_TPB), 0, d->stream, PpBaseStream<uint64_t>{(const uint64_t *)(in + at[0])}, P,
                               (uint64_t *)st.rec[0].p, (uint64_t *)st.val[0].p, bor);
    else hipLaunchKernelGGL((k_pp_records<false, PpBaseStream<uint32_t>>), dim3(nor), dim3(PP_TPB), 0, d->stream, PpBaseStream<uint32_t>{(const uint32_t *)(in + at[0])}, P,
                            (uint64_t *)st.rec[0].p, (uint64_t *)nullptr, bor);
    hipLaunchKernelGGL(k_pp_or_final, dim3(1), dim3(64), 0, d->stream, (const uint64_t *)bor, nor, bor + 2 * PP_OR_BLOCKS);
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, st.ev.record(1, d->stream));
    // the flags' counts, held against the stream sizes before anything is indexed by them
    HIP_TRY(d, sco_scan<true>(d->stream, ds.off16_flag, near_inc, P, PpIsOne{}, ScoPlus{}, 0u, sco_tmp));
    HIP_TRY(d, sco_scan<true>(d->stream, ds.del_flag, del_inc, nf, PpNonZero{}, ScoPlus{}, 0u, sco_tmp));
    HIP_TRY(d, st.ev.record(2, d->stream));
    uint64_t ors[2] = {0, 0};
    uint32_t n_near = 0, n_del = 0;
    HIP_TRY(d, hipMemcpyAsync(ors, bor + 2 * PP_OR_BLOCKS, 16, hipMemcpyDeviceToHost, d->stream));
    if (P) HIP_TRY(d, hipMemcpyAsync(&n_near, near_inc + P - 1, 4, hipMemcpyDeviceToHost, d->stream));
    if (nf) HIP_TRY(d, hipMemcpyAsync(&n_del, del_inc + nf - 1, 4, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    if (n_near != s->n_off16) return pp_fail(d, who, "off16_flag holds " + std::to_string(n_near) + " ones, n_off16 is " + std::to_string(s->n_off16));
    if (P - n_near != nf) return pp_fail(d, who, "off16_flag holds " + std::to_string(P - n_near) + " far pairs, n_delta_flag is " + std::to_string(nf));
    if (n_del != s->n_delta16) return pp_fail(d, who, "delta16_flag holds " + std::to_string(n_del) + " delta pairs, n_delta16 is " + std::to_string(s->n_delta16));
    if (nf - n_del != s->n_not_base) return pp_fail(d, who, "delta16_flag holds " + std::to_string(nf - n_del) + " full pairs, n_not_base is " + std::to_string(s->n_not_base));

    const uint64_t *a = nullptr, *b = nullptr;
    if ((e = pp_sort(d, st, W8, P, ors[0], &a, &b))) return e;
    HIP_TRY(d, st.ev.record(3, d->stream));
    if (P) hipLaunchKernelGGL((k_pp_dec_ops<W8>), dim3(pp_grid(P)), dim3(PP_TPB), 0, d->stream, a, b, P, ds, d_out, kind, val);
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, st.ev.record(4, d->stream));
    // refPrev at every ranked pair; the scan's last pass puts the delta pairs' mates in their places
    HIP_TRY(d, (sco_device_scan<true, false>(d->stream, PpChainIn{kind, val}, P, PpSegOp{}, PpSeg{0, 0u}, PpSeg{0, 0u}, PpDeltaSink<W8>{a, b, kind, P, d_out}, (PpSeg *)st.bsum.p)));
    HIP_TRY(d, st.ev.record(5, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    pgrc_pairpos_timing &t = st.tm;
    t = pgrc_pairpos_timing{};
    t.struct_size = sizeof(pgrc_pairpos_timing);
    t.encode = 0;
    t.ms_upload = ms_upload;
    t.ms_sort_device = st.ev.ms(0, 1) + st.ev.ms(2, 3);
    t.ms_scan_device = st.ev.ms(1, 2) + st.ev.ms(3, 4);
    t.ms_scatter_device = st.ev.ms(4, 5);
    t.bytes_up = up;
    t.n_near = n_near;
    t.n_delta = n_del;
    t.n_full = nf - n_del;
    return PGRC_OK;
}

int pgrc_pairpos_check_streams(PgrcStage *d, const pgrc_pairpos_streams *s) {
    static const char *who = "pair positions (decode)";
    if (!s || s->struct_size != sizeof(pgrc_pairpos_streams)) return pp_fail(d, who, "streams is NULL or struct_size is not sizeof(pgrc_pairpos_streams)");
    if (s->n_total & 1) return pp_fail(d, who, "n_total is odd");
    if (s->pos_width != 4 && s->pos_width != 8) return pp_fail(d, who, "pos_width must be 4 or 8");
    const uint64_t P = s->n_total / 2;
    if (P >= PP_MAX_PAIRS) return pp_fail(d, who, "too many pairs for the rank sort");
    if (P && (!s->base_pos || !s->off16_flag)) return pp_fail(d, who, "base_pos or off16_flag is NULL");
    if (s->n_off16 && (!s->off_base_first || !s->off_value)) return pp_fail(d, who, "off_base_first or off_value is NULL with n_off16 > 0");
    if (s->n_delta_flag && !s->delta16_flag) return pp_fail(d, who, "delta16_flag is NULL with n_delta_flag > 0");
    if (s->n_delta16 && (!s->delta_base_first || !s->delta_value)) return pp_fail(d, who, "delta_base_first or delta_value is NULL with n_delta16 > 0");
    if (s->n_not_base && !s->not_base_pos) return pp_fail(d, who, "not_base_pos is NULL with n_not_base > 0");
    // (counts beyond P cannot agree with the flags; refused here so that no buffer is sized by them)
    if (s->n_off16 > P || s->n_delta_flag > P || s->n_delta16 > P || s->n_not_base > P) return pp_fail(d, who, "a stream holds more elements than there are pairs");
    return PGRC_OK;
}

int pgrc_pairpos_decode_device(pgrc_decode_ctx *d, const pgrc_pairpos_streams *s, uint64_t *d_out) {
    int e;
    if ((e = pgrc_pairpos_check_streams(d, s))) return e;
    d->pp.have_timing = false;
    return s->pos_width == 8 ? pp_decode_run<true>(d, d->pp, s, d_out) : pp_decode_run<false>(d, d->pp, s, d_out);
}

typedef DecBlockLayout<8> PpEncOut;    // where the streams start in the output block, and their bytes
static PpEncOut pp_enc_layout(uint64_t P, uint64_t W, uint64_t n_near, uint64_t nf, uint64_t n_del, uint64_t n_full) {
    const uint64_t b[8] = {P * W, P, n_near, n_near * 2, nf, n_del, n_del * 2, n_full * W};
    return dec_block_layout(b);
}

// on_device: org_h is memory of the stage's device, complete when the call is made, and is read where it lies
template <bool W8>
static int pp_encode_run(PgrcStage *d, PgrcPairPos &st, const uint64_t *org_h, bool on_device, uint64_t T, pgrc_pairpos_streams *out) {
    static const char *who = "pair positions (encode)";
    const uint64_t P = T / 2, W = W8 ? 8 : 4;
    const auto t0 = std::chrono::steady_clock::now();
    int e;
    if ((e = st.ev.ensure(d)) || (e = pp_sort_buffers(d, st, W8, P))) return e;
    const PpEncOut dev = pp_enc_layout(P, W, P, P, P, P);        // on the device every stream has room for all pairs
    const uint64_t near_at = dec_a16(P * 8) + 16, bf_at = near_at + dec_a16(P * 4) + 16, rank_bytes = bf_at + P + 16;
    const uint64_t frank_at = dec_a16(P * 8) + 16, pre_at = frank_at + dec_a16(P * 4) + 16, dinc_at = pre_at + dec_a16(P * 4) + 16,
                   dval_at = dinc_at + dec_a16(P * 4) + 16, map_at = dval_at + dec_a16(P * 2) + 16, far_bytes = map_at + P + 16;
    const uint64_t bsum_bytes = dec_a16(sco_scratch_elems(P) * 4) + 2 * PP_OR_BLOCKS * 8 + 64;
    if ((e = pgrc_bufs_unpooled(d, {{&st.in, on_device ? 16 : T * 8 + 16}, {&st.rank, rank_bytes}, {&st.far, far_bytes}, {&st.out, dev.total}, {&st.bsum, bsum_bytes}})))
        return e;
    if (T && !on_device && (e = dec_upload(d, st.in.p, org_h, T * 8))) return e;
    const float ms_upload = dec_ms_since(t0);
    const uint64_t *org = on_device ? org_h : (const uint64_t *)st.in.p;
    uint8_t *rk = (uint8_t *)st.rank.p, *fr = (uint8_t *)st.far.p, *ob = (uint8_t *)st.out.p;
    uint64_t *rel = (uint64_t *)rk;
    uint32_t *near_inc = (uint32_t *)(rk + near_at);
    uint8_t *bf = rk + bf_at;
    uint64_t *far_rel = (uint64_t *)fr;
    uint32_t *far_rank = (uint32_t *)(fr + frank_at), *pre = (uint32_t *)(fr + pre_at), *del_inc = (uint32_t *)(fr + dinc_at);
    int16_t *dval = (int16_t *)(fr + dval_at);
    uint8_t *map = fr + map_at;
    uint8_t *off16_flag = ob + dev.at[1], *off_bf = ob + dev.at[2], *del_flag = ob + dev.at[4], *del_bf = ob + dev.at[5];
    uint16_t *off_val = (uint16_t *)(ob + dev.at[3]);
    int16_t *del_val = (int16_t *)(ob + dev.at[6]);
    void *not_base = ob + dev.at[7];
    uint64_t *bor = (uint64_t *)((uint8_t *)st.bsum.p + bsum_bytes - 2 * PP_OR_BLOCKS * 8 - 32);
    uint32_t *sco_tmp = (uint32_t *)st.bsum.p;

    HIP_TRY(d, st.ev.record(0, d->stream));
    const uint32_t nor = (uint32_t)std::min<uint64_t>(pp_grid(P), PP_OR_BLOCKS);
    hipLaunchKernelGGL((k_pp_records<W8, PpBaseOrg>), dim3(nor), dim3(PP_TPB), 0, d->stream, PpBaseOrg{org}, P, (uint64_t *)st.rec[0].p,
                       (uint64_t *)(W8 ? st.val[0].p : nullptr), bor);
    hipLaunchKernelGGL(k_pp_or_final, dim3(1), dim3(64), 0, d->stream, (const uint64_t *)bor, nor, bor + 2 * PP_OR_BLOCKS);
    HIP_TRY(d, hipGetLastError());
    uint64_t ors[2] = {0, 0};
    HIP_TRY(d, hipMemcpyAsync(ors, bor + 2 * PP_OR_BLOCKS, 16, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    if (!W8 && (ors[1] >> 32)) return pp_fail(d, who, "a position of 2^32 or more with pos_width 4");
    const uint64_t *a = nullptr, *b = nullptr;
    if ((e = pp_sort(d, st, W8, P, ors[0], &a, &b))) return e;
    HIP_TRY(d, st.ev.record(1, d->stream));
    uint32_t n_near = 0, n_del = 0;
    if (P) {
        hipLaunchKernelGGL((k_pp_enc_class<W8>), dim3(pp_grid(P)), dim3(PP_TPB), 0, d->stream, a, b, org, P, off16_flag, rel, bf);
        HIP_TRY(d, sco_scan<true>(d->stream, (const uint8_t *)off16_flag, near_inc, P, ScoIdentity{}, ScoPlus{}, 0u, sco_tmp));
        HIP_TRY(d, hipMemcpyAsync(&n_near, near_inc + P - 1, 4, hipMemcpyDeviceToHost, d->stream));
    }
    HIP_TRY(d, st.ev.record(2, d->stream));
    if (P) {
        if (W8) hipLaunchKernelGGL((k_pp_enc_base<uint64_t>), dim3(pp_grid(P)), dim3(PP_TPB), 0, d->stream, org, P, (uint64_t *)(ob + dev.at[0]));
        else hipLaunchKernelGGL((k_pp_enc_base<uint32_t>), dim3(pp_grid(P)), dim3(PP_TPB), 0, d->stream, org, P, (uint32_t *)(ob + dev.at[0]));
        hipLaunchKernelGGL(k_pp_enc_compact, dim3(pp_grid(P)), dim3(PP_TPB), 0, d->stream, P, (const uint8_t *)off16_flag, (const uint32_t *)near_inc, (const uint64_t *)rel,
                           (const uint8_t *)bf, off_bf, off_val, far_rel, far_rank);
    }
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, st.ev.record(3, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    const uint64_t nf = P - n_near;
    if (nf) {
        hipLaunchKernelGGL((k_pp_enc_maps<int16_t, uint64_t>), dim3(pp_grid(nf)), dim3(PP_TPB), 0, d->stream, nf, (const uint64_t *)far_rel, map);
        HIP_TRY(d, sco_scan<false>(d->stream, (const uint8_t *)map, pre, nf, ScoIdentity{}, PpCompose{}, PP_MAP_IDENT, sco_tmp));
        hipLaunchKernelGGL((k_pp_enc_kinds<int16_t, uint64_t>), dim3(pp_grid(nf)), dim3(PP_TPB), 0, d->stream, nf, (const uint64_t *)far_rel, (const uint32_t *)pre, del_flag, dval);
        HIP_TRY(d, sco_scan<true>(d->stream, (const uint8_t *)del_flag, del_inc, nf, ScoIdentity{}, ScoPlus{}, 0u, sco_tmp));
        HIP_TRY(d, hipMemcpyAsync(&n_del, del_inc + nf - 1, 4, hipMemcpyDeviceToHost, d->stream));
    }
    HIP_TRY(d, st.ev.record(4, d->stream));
    if (nf) hipLaunchKernelGGL((k_pp_enc_far<W8>), dim3(pp_grid(nf)), dim3(PP_TPB), 0, d->stream, nf, (const uint32_t *)far_rank, (const uint64_t *)far_rel,
                               (const uint8_t *)del_flag, (const uint32_t *)del_inc, (const int16_t *)dval, (const uint8_t *)bf, a, b, del_bf, del_val, not_base);
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, st.ev.record(5, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));

    // the streams, now that their sizes are known: one page-locked block
    const auto t1 = std::chrono::steady_clock::now();
    const PpEncOut h = pp_enc_layout(P, W, n_near, nf, n_del, nf - n_del);
    const void *src[8];
    for (int k = 0; k < 8; k++) src[k] = ob + dev.at[k];
    uint8_t *blk = nullptr;
    uint64_t down = 0;
    if ((e = dec_download_block(d, who, h, src, &blk, &down))) return e;
    *out = pgrc_pairpos_streams{};
    out->struct_size = sizeof(pgrc_pairpos_streams);
    out->pos_width = (uint32_t)W;
    out->n_total = T;
    out->base_pos = blk + h.at[0];
    out->off16_flag = blk + h.at[1];
    out->off_base_first = blk + h.at[2];
    out->off_value = (const uint16_t *)(blk + h.at[3]);
    out->delta16_flag = blk + h.at[4];
    out->delta_base_first = blk + h.at[5];
    out->delta_value = (const int16_t *)(blk + h.at[6]);
    out->not_base_pos = blk + h.at[7];
    out->n_off16 = n_near;
    out->n_delta_flag = nf;
    out->n_delta16 = n_del;
    out->n_not_base = nf - n_del;
    pgrc_pairpos_timing &t = st.tm;
    t = pgrc_pairpos_timing{};
    t.struct_size = sizeof(pgrc_pairpos_timing);
    t.encode = 1;
    t.ms_upload = ms_upload;
    t.ms_sort_device = st.ev.ms(0, 1);
    t.ms_scan_device = st.ev.ms(1, 2) + st.ev.ms(3, 4);
    t.ms_scatter_device = st.ev.ms(2, 3) + st.ev.ms(4, 5);
    t.ms_download = dec_ms_since(t1);
    t.ms_call = dec_ms_since(t0);
    t.bytes_up = on_device ? 0 : T * 8;
    t.bytes_down = down;
    t.n_near = n_near;
    t.n_delta = n_del;
    t.n_full = nf - n_del;
    st.have_timing = true;
    return PGRC_OK;
}

int pgrc_pairpos_encode_device(PgrcStage *d, PgrcPairPos &st, const uint64_t *d_org_idx_to_pos, uint64_t n_total, uint32_t pos_width, pgrc_pairpos_streams *out) {
    static const char *who = "pair positions (encode)";
    if (n_total & 1) return pp_fail(d, who, "n_total is odd");
    if (pos_width != 4 && pos_width != 8) return pp_fail(d, who, "pos_width must be 4 or 8");
    if (n_total / 2 >= PP_MAX_PAIRS) return pp_fail(d, who, "too many pairs for the rank sort");
    st.have_timing = false;
    return pos_width == 8 ? pp_encode_run<true>(d, st, d_org_idx_to_pos, true, n_total, out) : pp_encode_run<false>(d, st, d_org_idx_to_pos, true, n_total, out);
}

extern "C" {

int pgrc_pairpos_encode(pgrc_decode_ctx *d, const uint64_t *org_idx_to_pos, uint64_t n_total, uint32_t pos_width, pgrc_pairpos_streams *out) {
    static const char *who = "pair positions (encode)";
    if (!d) return PGRC_E_PARAM;
    if (!out) return pp_fail(d, who, "out is NULL");
    if (n_total & 1) return pp_fail(d, who, "n_total is odd");
    if (pos_width != 4 && pos_width != 8) return pp_fail(d, who, "pos_width must be 4 or 8");
    if (n_total && !org_idx_to_pos) return pp_fail(d, who, "org_idx_to_pos is NULL");
    if (n_total / 2 >= PP_MAX_PAIRS) return pp_fail(d, who, "too many pairs for the rank sort");
    PGRC_ON_DEVICE(d);
    d->pp.have_timing = false;
    return pos_width == 8 ? pp_encode_run<true>(d, d->pp, org_idx_to_pos, false, n_total, out) : pp_encode_run<false>(d, d->pp, org_idx_to_pos, false, n_total, out);
}

void pgrc_pairpos_free(pgrc_pairpos_streams *s) {
    if (!s) return;
    if (s->base_pos) (void)hipHostFree(const_cast<void *>(s->base_pos));
    *s = pgrc_pairpos_streams{};
}

int pgrc_pairpos_decode(pgrc_decode_ctx *d, const pgrc_pairpos_streams *s, uint64_t *pg_pos) {
    if (!d) return PGRC_E_PARAM;
    if (s && s->n_total && !pg_pos) return pp_fail(d, "pair positions (decode)", "pg_pos is NULL");
    PGRC_ON_DEVICE(d);
    const auto t0 = std::chrono::steady_clock::now();
    int e;
    if ((e = pgrc_pairpos_check_streams(d, s))) return e;
    if ((e = pgrc_buf_unpooled(d, d->pp.out, s->n_total * 8 + 16))) return e;
    if ((e = pgrc_pairpos_decode_device(d, s, (uint64_t *)d->pp.out.p))) return e;
    const auto t1 = std::chrono::steady_clock::now();
    if ((e = dec_download_host(d, pg_pos, d->pp.out.p, s->n_total * 8))) return e;
    d->pp.tm.ms_download = dec_ms_since(t1);
    d->pp.tm.bytes_down = s->n_total * 8;
    d->pp.tm.ms_call = dec_ms_since(t0);
    d->pp.have_timing = true;
    return PGRC_OK;
}

int pgrc_pairpos_get_timing(pgrc_decode_ctx *d, pgrc_pairpos_timing *out) {
    if (!d) return PGRC_E_PARAM;
    if (!out || out->struct_size != sizeof(pgrc_pairpos_timing)) return dec_fail(d, PGRC_E_PARAM, "timing is NULL or struct_size is not sizeof(pgrc_pairpos_timing)");
    if (!d->pp.have_timing) return dec_fail(d, PGRC_E_STATE, "no pair-position call has succeeded on this context");
    *out = d->pp.tm;
    return PGRC_OK;
}

}   // extern "C"
