// pairorder.hip -- the pair-order coding of the paired mode that does not preserve the order, on the device: the encoder's
// SeparatedPseudoGenomePersistence::compressReadsOrder (SeparatedPseudoGenomePersistence.cpp:220-339; include/pgrc_decode.h,
// "The pair-order coding") and, in the second half of this file, the decoder's decompressReadsOrder
// (:341-443; include/pgrc_pairorder_decode.h).
//
// The reference's loop walks the T entries of the joined reads lists, skips the ones an earlier entry has marked as its mate,
// and codes mate - entry for the others with the three scalars of compressReadsPgPositions.  Here it falls apart into
//   rev                            one scatter: rev[org[i]] = i (values >= T refused; a duplicate loses its slot and is found by
//                                  the read-back rev[org[i]] == i in the next kernel)
//   mate, base, rel                one 8-byte gather per entry: rev[org[i]] and rev[org[i] ^ 1] are neighbours.  An entry is a
//                                  base iff its mate lies after it; rel = mate - i, 0 for the other entries
//   pair numbers                   scanops.h over rel != 0; the bases go to pair order, and revPairBaseOrgIdx is one scatter
//   near / far, delta / full       as pairpos.hip's encoder: a scan of the near flags, far pairs into far order, ppchain.h's
//                                  maps -> scan with PpCompose -> kinds with int8 deltas, a scan of the delta flags
// Integer work bound by two random 4- / 8-byte accesses per entry and HBM streams; no atomics, no library kernel.
#include "ppchain.h"
#include "rlistctx.h"

// ------------------------------------------------------------------------------------------------ kernels
// bad[0]: a value >= T was seen
static __global__ void __launch_bounds__(PP_TPB) k_po_scatter(const uint32_t *__restrict__ org, uint64_t T, uint32_t *__restrict__ rev, uint32_t *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (i >= T) return;
    const uint32_t v = org[i];
    if (v >= T) {
        bad[0] = 1;
        return;
    }
    rev[v] = (uint32_t)i;
}

struct PoNonZero { __device__ uint32_t operator()(uint32_t x) const { return x ? 1u : 0u; } };

// rel[i] = mate - i for a base, 0 otherwise (:266-272); bad[1]: an entry does not find itself in rev (its value occurs twice)
static __global__ void __launch_bounds__(PP_TPB) k_po_class(const uint32_t *__restrict__ org, uint64_t T, const uint32_t *__restrict__ rev, uint32_t *__restrict__ rel,
                                                            uint32_t *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (i >= T) return;
    const uint32_t v = org[i];
    uint32_t r = 0;
    if (v < T) {        // (T is even: v ^ 1 < T as well)
        const uint2 two = *(const uint2 *)(rev + (v & ~1u));
        const uint32_t self = (v & 1u) ? two.y : two.x, mate = (v & 1u) ? two.x : two.y;
        if (self != (uint32_t)i) bad[1] = 1;
        if (mate > (uint32_t)i) r = mate - (uint32_t)i;
    }
    rel[i] = r;
}

// the bases into pair order: rel, the near flag (offsetInUint8Flag itself), the base's file; revPairBaseOrgIdx (:271)
static __global__ void __launch_bounds__(PP_TPB) k_po_pairs(const uint32_t *__restrict__ org, uint64_t T, const uint32_t *__restrict__ rel, const uint32_t *__restrict__ base_inc,
                                                            uint32_t *__restrict__ prel, uint8_t *__restrict__ off8_flag, uint8_t *__restrict__ pfile,
                                                            uint32_t *__restrict__ pair_base_org_idx) {
    const uint64_t i = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (i >= T) return;
    const uint32_t r = rel[i];
    if (!r) return;
    const uint32_t k = base_inc[i] - 1u, v = org[i];
    prel[k] = r;
    off8_flag[k] = r <= 255u ? 1 : 0;
    if (pfile) pfile[k] = (uint8_t)(v & 1u);
    if (pair_base_org_idx) pair_base_org_idx[v >> 1] = 2u * k + (v & 1u);
}

// near pairs -> their value (and file flag); far pairs -> far order (and their file flag)
static __global__ void __launch_bounds__(PP_TPB) k_po_compact(uint64_t P, const uint8_t *__restrict__ off8_flag, const uint32_t *__restrict__ near_inc,
                                                              const uint32_t *__restrict__ prel, const uint8_t *__restrict__ pfile, uint8_t *__restrict__ off_val,
                                                              uint8_t *__restrict__ off_file, uint32_t *__restrict__ far_rel, uint8_t *__restrict__ nonoff_file) {
    const uint64_t k = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (k >= P) return;
    const uint32_t ninc = near_inc[k];
    if (off8_flag[k]) {
        off_val[ninc - 1u] = (uint8_t)prel[k];
        if (pfile) off_file[ninc - 1u] = pfile[k];
    } else {
        far_rel[k - ninc] = prel[k];
        if (pfile) nonoff_file[k - ninc] = pfile[k];
    }
}

static __global__ void __launch_bounds__(PP_TPB) k_po_far(uint64_t nf, const uint32_t *__restrict__ far_rel, const uint8_t *__restrict__ del_flag,
                                                          const uint32_t *__restrict__ del_inc, const int8_t *__restrict__ dval, int8_t *__restrict__ del_val,
                                                          uint32_t *__restrict__ full) {
    const uint64_t k = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (k >= nf) return;
    const uint32_t dinc = del_inc[k];
    if (del_flag[k]) del_val[dinc - 1u] = dval[k];
    else full[k - dinc] = far_rel[k];
}

// ------------------------------------------------------------------------------------------------ host side
static int po_fail(PgrcStage *d, const std::string &msg) { return dec_fail(d, PGRC_E_PARAM, "pair order (encode): " + msg); }

// the nine streams in the order of pgrc_pairorder_streams: where they start in a block, and their bytes
enum { PO_OFF8, PO_OFFV, PO_DELF, PO_DELV, PO_FULL, PO_PBO, PO_OFFF, PO_NONF, PO_REV, PO_NS };
typedef DecBlockLayout<PO_NS> PoLayout;
static PoLayout po_layout(int32_t form, uint64_t T, uint64_t n_near, uint64_t nf, uint64_t n_del, uint64_t n_full) {
    const uint64_t P = T / 2;
    const bool coded = form != PGRC_PAIRORDER_COMPLETE_SINGLE_FILE, ff = form == PGRC_PAIRORDER_FILE_FLAGS;
    const uint64_t b[PO_NS] = {coded ? P : 0, n_near, nf, n_del, n_full * 4, form == PGRC_PAIRORDER_COMPLETE ? P * 4 : 0, ff ? n_near : 0, ff ? nf : 0, coded ? 0 : T * 4};
    return dec_block_layout(b);
}

// d_joined: the joined array in memory of the stage's device, complete when the call is made (pgrc_pairorder_encode_joined);
// NULL: the three host lists go up into the state's `in`
static int po_encode_run(PgrcStage *d, PgrcPairOrder &st, const uint32_t *const org_h[3], const uint64_t n[3], const uint32_t *d_joined, uint64_t T, int32_t form, pgrc_pairorder_streams *out) {
    const uint64_t P = T / 2;
    const bool coded = form != PGRC_PAIRORDER_COMPLETE_SINGLE_FILE, ff = form == PGRC_PAIRORDER_FILE_FLAGS, complete = form == PGRC_PAIRORDER_COMPLETE;
    const auto t0 = std::chrono::steady_clock::now();
    int e;
    if ((e = st.ev.ensure(d))) return e;
    const PoLayout dev = po_layout(form, T, P, P, P, P);         // on the device every stream has room for all pairs
    const uint64_t binc_at = dec_a16(T * 4) + 16, ent_bytes = binc_at + T * 4 + 16;
    const uint64_t file_at = dec_a16(P * 4) + 16, ninc_at = file_at + dec_a16(P) + 16, frel_at = ninc_at + dec_a16(P * 4) + 16, pre_at = frel_at + dec_a16(P * 4) + 16,
                   dinc_at = pre_at + dec_a16(P * 4) + 16, dval_at = dinc_at + dec_a16(P * 4) + 16, map_at = dval_at + dec_a16(P) + 16, pair_bytes = map_at + P + 16;
    const uint64_t sco_bytes = dec_a16(sco_scratch_elems(T) * 4), bsum_bytes = sco_bytes + 32;
    if ((e = pgrc_bufs_unpooled(d, {{&st.in, d_joined ? 16 : T * 4 + 16}, {&st.rev, T * 4 + 16}, {&st.ent, ent_bytes}, {&st.pair, coded ? pair_bytes : 16},
                                    {&st.out, dev.total}, {&st.bsum, bsum_bytes}})))
        return e;
    const uint32_t *org = d_joined ? d_joined : (const uint32_t *)st.in.p;
    uint32_t *rev = (uint32_t *)st.rev.p;
    uint8_t *en = (uint8_t *)st.ent.p, *pr = (uint8_t *)st.pair.p, *ob = (uint8_t *)st.out.p;
    uint32_t *rel = (uint32_t *)en, *base_inc = (uint32_t *)(en + binc_at);
    uint32_t *sco_tmp = (uint32_t *)st.bsum.p, *bad = (uint32_t *)((uint8_t *)st.bsum.p + sco_bytes);
    // the three lists one after the other, as the reads lists number their entries
    uint64_t first = 0;
    for (int l = 0; l < 3 && !d_joined; l++) {
        if (n[l] && (e = dec_upload(d, (uint32_t *)st.in.p + first, org_h[l], n[l] * 4))) return e;
        first += n[l];
    }
    HIP_TRY(d, st.ev.record(0, d->stream));
    if (T) HIP_TRY(d, hipMemsetAsync(rev, 0xFF, T * 4, d->stream));      // the sentinel: no entry index (T <= 2^32 - 2)
    HIP_TRY(d, hipMemsetAsync(bad, 0, 16, d->stream));
    const float ms_upload = dec_ms_since(t0);

    uint32_t h_bad[2] = {0, 0}, n_base = 0, n_near = 0, n_del = 0;
    if (T) {
        hipLaunchKernelGGL(k_po_scatter, dim3(pp_grid(T)), dim3(PP_TPB), 0, d->stream, (const uint32_t *)org, T, rev, bad);
        HIP_TRY(d, st.ev.record(10, d->stream));
        hipLaunchKernelGGL(k_po_class, dim3(pp_grid(T)), dim3(PP_TPB), 0, d->stream, (const uint32_t *)org, T, (const uint32_t *)rev, rel, bad);
        HIP_TRY(d, hipGetLastError());
    }
    HIP_TRY(d, st.ev.record(1, d->stream));
    if (T && coded) {
        HIP_TRY(d, sco_scan<true>(d->stream, (const uint32_t *)rel, base_inc, T, PoNonZero{}, ScoPlus{}, 0u, sco_tmp));
        HIP_TRY(d, hipMemcpyAsync(&n_base, base_inc + T - 1, 4, hipMemcpyDeviceToHost, d->stream));
    }
    HIP_TRY(d, st.ev.record(2, d->stream));
    HIP_TRY(d, hipMemcpyAsync(h_bad, bad, 8, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    // nothing below is indexed by a pair number before the input is known to be a permutation
    if (h_bad[0]) return po_fail(d, "an original index of " + std::to_string(T) + " (the entries' count) or more");
    if (h_bad[1]) return po_fail(d, "an original index occurs twice");
    if (coded && n_base != P) return dec_fail(d, PGRC_E_DEVICE, "pair order (encode): " + std::to_string(n_base) + " bases among " + std::to_string(T) + " entries");

    uint32_t *prel = (uint32_t *)pr, *near_inc = (uint32_t *)(pr + ninc_at), *far_rel = (uint32_t *)(pr + frel_at), *pre = (uint32_t *)(pr + pre_at),
             *del_inc = (uint32_t *)(pr + dinc_at);
    uint8_t *pfile = ff ? pr + file_at : nullptr, *map = pr + map_at;
    int8_t *dval = (int8_t *)(pr + dval_at);
    uint8_t *off8_flag = ob + dev.at[PO_OFF8], *off_val = ob + dev.at[PO_OFFV], *del_flag = ob + dev.at[PO_DELF];
    int8_t *del_val = (int8_t *)(ob + dev.at[PO_DELV]);
    uint32_t *full = (uint32_t *)(ob + dev.at[PO_FULL]), *pbo = complete ? (uint32_t *)(ob + dev.at[PO_PBO]) : nullptr;
    uint8_t *off_file = ff ? ob + dev.at[PO_OFFF] : nullptr, *nonoff_file = ff ? ob + dev.at[PO_NONF] : nullptr;
    const bool pairs = coded && P;
    HIP_TRY(d, st.ev.record(8, d->stream));         // (the host's wait above is no device time)
    if (pairs) hipLaunchKernelGGL(k_po_pairs, dim3(pp_grid(T)), dim3(PP_TPB), 0, d->stream, (const uint32_t *)org, T, (const uint32_t *)rel, (const uint32_t *)base_inc, prel,
                                  off8_flag, pfile, pbo);
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, st.ev.record(3, d->stream));
    if (pairs) {
        HIP_TRY(d, sco_scan<true>(d->stream, (const uint8_t *)off8_flag, near_inc, P, ScoIdentity{}, ScoPlus{}, 0u, sco_tmp));
        HIP_TRY(d, hipMemcpyAsync(&n_near, near_inc + P - 1, 4, hipMemcpyDeviceToHost, d->stream));
    }
    HIP_TRY(d, st.ev.record(4, d->stream));
    if (pairs) hipLaunchKernelGGL(k_po_compact, dim3(pp_grid(P)), dim3(PP_TPB), 0, d->stream, P, (const uint8_t *)off8_flag, (const uint32_t *)near_inc, (const uint32_t *)prel,
                                  (const uint8_t *)pfile, off_val, off_file, far_rel, nonoff_file);
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, st.ev.record(5, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    const uint64_t nf = pairs ? P - n_near : 0;
    HIP_TRY(d, st.ev.record(9, d->stream));
    if (nf) {
        hipLaunchKernelGGL((k_pp_enc_maps<int8_t, uint32_t>), dim3(pp_grid(nf)), dim3(PP_TPB), 0, d->stream, nf, (const uint32_t *)far_rel, map);
        HIP_TRY(d, sco_scan<false>(d->stream, (const uint8_t *)map, pre, nf, ScoIdentity{}, PpCompose{}, PP_MAP_IDENT, sco_tmp));
        hipLaunchKernelGGL((k_pp_enc_kinds<int8_t, uint32_t>), dim3(pp_grid(nf)), dim3(PP_TPB), 0, d->stream, nf, (const uint32_t *)far_rel, (const uint32_t *)pre, del_flag, dval);
        HIP_TRY(d, sco_scan<true>(d->stream, (const uint8_t *)del_flag, del_inc, nf, ScoIdentity{}, ScoPlus{}, 0u, sco_tmp));
        HIP_TRY(d, hipMemcpyAsync(&n_del, del_inc + nf - 1, 4, hipMemcpyDeviceToHost, d->stream));
    }
    HIP_TRY(d, st.ev.record(6, d->stream));
    if (nf) hipLaunchKernelGGL(k_po_far, dim3(pp_grid(nf)), dim3(PP_TPB), 0, d->stream, nf, (const uint32_t *)far_rel, (const uint8_t *)del_flag, (const uint32_t *)del_inc,
                               (const int8_t *)dval, del_val, full);
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, st.ev.record(7, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));

    // the streams, now that their sizes are known: one page-locked block
    const auto t1 = std::chrono::steady_clock::now();
    const PoLayout h = po_layout(form, T, n_near, nf, n_del, nf - n_del);
    const void *src[PO_NS] = {off8_flag, off_val, del_flag, del_val, full, ob + dev.at[PO_PBO], ob + dev.at[PO_OFFF], ob + dev.at[PO_NONF], rev};
    uint8_t *blk = nullptr;
    uint64_t down = 0;
    if ((e = dec_download_block(d, "pair order (encode)", h, src, &blk, &down))) return e;
    out->struct_size = sizeof(pgrc_pairorder_streams);
    out->form = form;
    out->n_total = T;
    out->off8_flag = blk;
    if (coded) {
        out->off_value = blk + h.at[PO_OFFV];
        out->delta8_flag = blk + h.at[PO_DELF];
        out->delta_value = (const int8_t *)(blk + h.at[PO_DELV]);
        out->full_offset = (const uint32_t *)(blk + h.at[PO_FULL]);
        if (complete) out->pair_base_org_idx = (const uint32_t *)(blk + h.at[PO_PBO]);
        if (ff) {
            out->off_base_file_flag = blk + h.at[PO_OFFF];
            out->nonoff_base_file_flag = blk + h.at[PO_NONF];
        }
    } else {
        out->rev = (const uint32_t *)(blk + h.at[PO_REV]);
    }
    out->n_off8 = n_near;
    out->n_delta_flag = nf;
    out->n_delta8 = n_del;
    out->n_full = nf - n_del;
    pgrc_pairorder_timing &t = st.tm;
    t = pgrc_pairorder_timing{};
    t.struct_size = sizeof(pgrc_pairorder_timing);
    t.form = form;
    t.ms_upload = ms_upload;
    t.ms_inverse_device = st.ev.ms(0, 1);
    t.ms_scatter_device = T ? st.ev.ms(0, 10) : 0;
    t.ms_scan_device = st.ev.ms(1, 2) + st.ev.ms(3, 4) + st.ev.ms(9, 6);
    t.ms_compact_device = st.ev.ms(8, 3) + st.ev.ms(4, 5) + st.ev.ms(6, 7);
    t.ms_download = dec_ms_since(t1);
    t.ms_call = dec_ms_since(t0);
    t.bytes_up = d_joined ? 0 : T * 4;
    t.bytes_down = down;
    t.n_near = n_near;
    t.n_delta = n_del;
    t.n_full = nf - n_del;
    st.have_timing = true;
    return PGRC_OK;
}

int pgrc_pairorder_encode_joined(PgrcStage *d, PgrcPairOrder &st, const uint32_t *d_joined, uint64_t T, int32_t form, pgrc_pairorder_streams *out) {
    *out = pgrc_pairorder_streams{};
    if (form < PGRC_PAIRORDER_IGNORE || form > PGRC_PAIRORDER_COMPLETE_SINGLE_FILE) return po_fail(d, "unknown form " + std::to_string(form));
    if (T >= (1ull << 32)) return po_fail(d, "2^32 entries or more");
    if (T & 1) return po_fail(d, "the entries' count is odd");
    st.have_timing = false;
    const int e = po_encode_run(d, st, nullptr, nullptr, d_joined, T, form, out);
    if (e) *out = pgrc_pairorder_streams{};
    return e;
}

// ================================================================================================ the decoder
// decompressReadsOrder (:341-443).  Every pair's offset d[k] comes from flag scans and ppchain.h's segmented
// sum; the forms' tails are a predicated swap and a gather; what is left is the landing: pair k's base is the k-th entry
// ("slot") that no earlier pair has marked as its mate.  A slot's kind depends only on marks made by bases before it, so ONE
// wave walks the slots in words of 64, lanes = slots, with k (pairs placed) and the word's incoming marks E:
//   settle   M = E; repeat: opens = ~M, lane j's pair = k + popc(opens below j), M' = E | {j + d < 64 of the open lanes};
//            M' == M ends it.  If M and M' agree below bit x, M is final below x and M' at x (induction over the slots: a
//            slot's bit in M' is computed from the bases before it, which are final with their final pair numbers).  So the
//            open lanes below x are final bases with their final pairs and their marks are final wherever they fall, and the
//            next M is E | the marks of the open lanes below x (which holds all of M' up to x: a mark lies behind its base).
//            The marks of the other lanes were computed from pair numbers that are still moving and are left out.  The final
//            prefix grows with every round: 64 rounds always suffice, the loop is capped there, and an unchanged M is the
//            reference's word.
//   commit   every open lane stores its pair and sends its mark when it lies beyond the word: below 3 batches ahead into a
//            bit ring of 4 batches in LDS, else into a bitmap in device memory (a relaxed atomic OR whose result nobody reads).
//            On entering batch m the workgroup ORs the bitmap's words of batch m into the ring and clears the ring's quarter
//            of batch m - 1: a bitmap mark on batch m was made 3 batches earlier or more, in front of a barrier (whose
//            workgroup-scope release and acquire order it before the merge's loads: writer and readers are one workgroup).
// The other three waves stage d for the sweep in LDS: while the sweep walks the chunk that starts at pair k0 they load pairs
// [k0 + C, k0 + 2C) into a ring of 2C (a chunk of C slots takes at most C pairs, so the next chunk finds its C pairs there).
// The sweep's critical path is LDS and cross-lane work; every loop has a bound fixed at launch, and the only waits are the
// workgroup's barriers, which every wave reaches.  Nothing here trusts d: every index is checked or reduced, and what does not
// fit sets a bit of the error word.
#define POD_TPB 256
#define POD_CHUNK 4096u                                     // slots of a chunk: 64 words between two barriers
#define POD_BATCH PGRC_PAIRORDER_DECODE_BATCH
#define POD_RING_WORDS (4u * POD_BATCH / 32u)               // u32 words of the mark ring (8 KB)
#define POD_BATCH_WORDS (POD_BATCH / 32u)
static_assert(POD_BATCH % POD_CHUNK == 0 && (POD_CHUNK & (POD_CHUNK - 1)) == 0 && POD_CHUNK % 64 == 0, "whole chunks in a batch, whole words in a chunk");

#define POD_E_OFFSET 1u         // a decoded offset below 1
#define POD_E_MATE 2u           // a mate at slot T or beyond
#define POD_E_PAIRS 4u          // an unmarked slot after the last pair was placed
#define POD_E_SLOTS 8u          // the slots ran out before the pairs did
#define POD_E_ROUNDS 16u        // a word did not settle in 64 rounds (impossible: see above)
#define POD_E_PERM 32u          // the landed array is no permutation in base order
#define POD_E_PBO 64u           // a pair_base_org_idx value of T or more

struct PoDecStreams {
    const uint8_t *off8_flag, *off_val, *del_flag;
    const int8_t *del_val;
    const uint32_t *full;
    const uint32_t *near_inc, *del_inc;      // inclusive counts of near pairs (pair order) / delta pairs (far order)
};

// the chain's entry of pair k: near pairs and full pairs after a delta pair (refPrev stays, :405) add nothing
struct PoChainIn {
    PoDecStreams s;
    __device__ PpSeg operator()(uint64_t k) const {
        if (s.off8_flag[k]) return PpSeg{0, 0u};
        const uint64_t f = k - s.near_inc[k];
        if (s.del_flag[f]) return PpSeg{s.del_val[s.del_inc[f] - 1u], 0u};
        if (f > 0 && s.del_flag[f - 1]) return PpSeg{0, 0u};
        return PpSeg{(int64_t)s.full[f - s.del_inc[f]], 1u};
    }
};

// every pair's offset as u32: 0 stands for "below 1" (flagged), 0xFFFFFFFF for anything that large or larger (no such mate)
struct PoOffsetSink {
    PoDecStreams s;
    uint32_t *d, *err;
    __device__ void operator()(uint64_t k, PpSeg acc) const {
        int64_t v;
        if (s.off8_flag[k]) {
            v = s.off_val[s.near_inc[k] - 1u];
        } else {
            const uint64_t f = k - s.near_inc[k];
            v = s.del_flag[f] ? acc.v : (int64_t)s.full[f - s.del_inc[f]];
        }
        if (v < 1) {
            atomicOr(err, POD_E_OFFSET);
            v = 0;
        }
        d[k] = v > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)v;
    }
};

// gmark: a bitmap of whole batches of slots, zero on entry; stat[0], stat[1]: words settled, rounds
static __global__ void __launch_bounds__(POD_TPB) k_po_land(const uint32_t *__restrict__ d, uint64_t P, uint32_t *__restrict__ pe, uint32_t *__restrict__ gmark,
                                                            uint32_t *__restrict__ err, uint64_t *__restrict__ stat) {
    __shared__ uint32_t ring[POD_RING_WORDS];
    __shared__ uint32_t dst[2 * POD_CHUNK];
    __shared__ uint32_t hit[64];            // the marks that fall into the word: per slot the lowest lane that marks it (64: none); read and reset by its own lane
    __shared__ uint64_t s_k[2];             // pairs placed when chunk c starts, at [c & 1]: written while the others may still read the other one
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t T = 2 * P, nchunks = (T + POD_CHUNK - 1) / POD_CHUNK;
    for (uint32_t w = tid; w < POD_RING_WORDS; w += POD_TPB) ring[w] = 0;
    for (uint32_t i = tid; i < POD_CHUNK; i += POD_TPB) dst[i] = i < P ? d[i] : 0u;
    if (tid < 64) hit[tid] = 64;
    if (tid == 0) s_k[0] = 0;
    __syncthreads();
    uint64_t k = 0, words = 0, rounds = 0;      // (wave 0's)
    uint32_t bad = 0;
    for (uint64_t c = 0; c < nchunks; c++) {
        const uint64_t k0 = s_k[c & 1];
        if (k0 >= P) break;                     // every thread reads the same k0: all leave together
        if (c % (POD_BATCH / POD_CHUNK) == 0) {
            const uint64_t m = c / (POD_BATCH / POD_CHUNK);
            for (uint32_t w = tid; w < POD_BATCH_WORDS; w += POD_TPB) {
                const uint32_t g = __hip_atomic_load(gmark + m * POD_BATCH_WORDS + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ring[(uint32_t)(m & 3u) * POD_BATCH_WORDS + w] |= g;
                ring[(uint32_t)((m + 3u) & 3u) * POD_BATCH_WORDS + w] = 0;
            }
            __syncthreads();
        }
        if (wave == 0) {
            k = k0;
            for (uint32_t wi = 0; wi < POD_CHUNK / 64; wi++) {
                const uint64_t slot0 = c * POD_CHUNK + (uint64_t)wi * 64;
                if (slot0 >= T || k >= P || bad) break;
                const uint32_t rw = (uint32_t)(slot0 / 32) % POD_RING_WORDS;
                uint64_t E = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(ring[rw]) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(ring[rw + 1]) << 32;      // (the builtin returns int)
                if (T - slot0 < 64) E |= ~0ull << (T - slot0);          // past the end: no slot
                uint64_t M = E;
                uint32_t dd = 0, isopen = 0;
                uint64_t kk = 0;
                bool settled = false;
                for (uint32_t r = 0; r < 64; r++) {
                    rounds++;
                    const uint64_t opens = ~M;
                    isopen = (uint32_t)(opens >> lane) & 1u;
                    kk = k + __builtin_amdgcn_mbcnt_hi((uint32_t)(opens >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)opens, 0u));
                    dd = (isopen && kk < P) ? dst[kk & (2 * POD_CHUNK - 1)] : 0u;
                    // (one wave's LDS accesses are served in order; the wave barriers keep the compiler from moving them)
                    if (isopen && dd && dd < 64u - lane) atomicMin(&hit[lane + dd], lane);
                    __builtin_amdgcn_wave_barrier();
                    const uint32_t src = __hip_atomic_load(&hit[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_store(&hit[lane], 64u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __builtin_amdgcn_wave_barrier();
                    const uint64_t Mn = E | __ballot(src < 64u);
                    if (Mn == M) {
                        settled = true;
                        break;
                    }
                    M = E | __ballot(src < (uint32_t)__builtin_ctzll(Mn ^ M));      // the marks of the final bases
                }
                if (!settled) {
                    bad = POD_E_ROUNDS;
                    break;
                }
                words++;
                if (isopen) {
                    const uint64_t slot = slot0 + lane, mate = slot + dd;
                    uint32_t e = 0;
                    if (kk >= P) e = POD_E_PAIRS;
                    else if (!dd) e = POD_E_OFFSET;
                    else if (mate >= T) e = POD_E_MATE;
                    else {
                        *(uint2 *)(pe + 2 * kk) = make_uint2((uint32_t)slot, (uint32_t)mate);
                        if (dd >= 64u - lane) {
                            if (dd < 3u * POD_BATCH) atomicOr(&ring[(uint32_t)(mate / 32) % POD_RING_WORDS], 1u << (mate & 31u));
                            else __hip_atomic_fetch_or(gmark + mate / 32, 1u << (mate & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                    if (e) atomicOr(err, e);
                }
                __builtin_amdgcn_wave_barrier();        // the ring's marks stay in front of the next word's read: LDS serves one wave in order, and
                                                        // nothing waits for the stores to pe or the bitmap
                k = min(k + (uint64_t)__popcll(~M), P);
            }
            if (bad) k = P;                     // (stops everything)
            if (lane == 0) s_k[(c + 1) & 1] = k;
            // The bitmap's marks reach the batch that merges them through the barrier's own release and acquire: the readers
            // are this workgroup's waves, so no wider fence -- which would write the L2 back chunk after chunk -- is needed.
            // At a batch's end the wave also waits until its atomics have been performed, so that nothing rests on the order
            // in which the CU's memory path serves two waves.
            if ((c + 1) % (POD_BATCH / POD_CHUNK) == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            // pairs [k0 + C, k0 + 2C) for the next chunk, while the sweep reads [k0, k0 + C)
            for (uint32_t i = tid - 64; i < POD_CHUNK; i += POD_TPB - 64) {
                const uint64_t q = k0 + POD_CHUNK + i;
                dst[q & (2 * POD_CHUNK - 1)] = q < P ? d[q] : 0u;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (bad) atomicOr(err, bad);
        else if (k < P) atomicOr(err, POD_E_SLOTS);
        stat[0] = words;
        stat[1] = rounds;
    }
}

// the landed array is a permutation of [0, T) in base order: every entry sets its bit (counted afterwards); the bases ascend
// and every mate lies after its base
static __global__ void __launch_bounds__(PP_TPB) k_po_check(const uint32_t *__restrict__ pe, uint64_t P, uint32_t *__restrict__ seen, uint32_t *__restrict__ err) {
    const uint64_t k = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (k >= P) return;
    const uint2 v = *(const uint2 *)(pe + 2 * k);
    const uint64_t T = 2 * P;
    bool ok = v.y > v.x && v.y < T && (k == 0 || pe[2 * k - 2] < v.x);
    if (ok) {
        __hip_atomic_fetch_or(seen + v.x / 32, 1u << (v.x & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_or(seen + v.y / 32, 1u << (v.y & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        atomicOr(err, POD_E_PERM);
    }
}

static __global__ void __launch_bounds__(PP_TPB) k_po_count(const uint32_t *__restrict__ seen, uint64_t nw, unsigned long long *__restrict__ count) {
    uint32_t c = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x; w < nw; w += (uint64_t)gridDim.x * PP_TPB) c += __popc(seen[w]);
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, (unsigned long long)c);
}

// FILE_FLAGS (:433-440): pair k is swapped iff its file flag is set
static __global__ void __launch_bounds__(PP_TPB) k_po_tail_flags(uint64_t P, const uint8_t *__restrict__ off8_flag, const uint32_t *__restrict__ near_inc,
                                                                 const uint8_t *__restrict__ off_file, const uint8_t *__restrict__ nonoff_file, uint32_t *__restrict__ out) {
    const uint64_t k = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (k >= P) return;
    const uint32_t ninc = near_inc[k];
    if (off8_flag[k] ? off_file[ninc - 1u] : nonoff_file[k - ninc]) {
        const uint2 v = *(const uint2 *)(out + 2 * k);
        *(uint2 *)(out + 2 * k) = make_uint2(v.y, v.x);
    }
}

// COMPLETE (:420-424): out[2p] = pe[r], out[2p + 1] = pe[r ^ 1] with r = revPairBaseOrgIdx[p]
static __global__ void __launch_bounds__(PP_TPB) k_po_tail_complete(uint64_t P, const uint32_t *__restrict__ pbo, const uint32_t *__restrict__ pe, uint32_t *__restrict__ out,
                                                                    uint32_t *__restrict__ err) {
    const uint64_t p = (uint64_t)blockIdx.x * PP_TPB + threadIdx.x;
    if (p >= P) return;
    const uint32_t r = pbo[p];
    if (r >= 2 * P) {
        atomicOr(err, POD_E_PBO);
        return;
    }
    *(uint2 *)(out + 2 * p) = make_uint2(pe[r], pe[r ^ 1u]);
}

static int pod_fail(PgrcStage *d, const std::string &msg) { return dec_fail(d, PGRC_E_PARAM, "pair order (decode): " + msg); }

int pgrc_pairorder_check_streams(PgrcStage *d, const pgrc_pairorder_streams *s) {
    if (!s || s->struct_size != sizeof(pgrc_pairorder_streams)) return pod_fail(d, "streams is NULL or struct_size is not sizeof(pgrc_pairorder_streams)");
    if (s->form < PGRC_PAIRORDER_IGNORE || s->form > PGRC_PAIRORDER_COMPLETE_SINGLE_FILE) return pod_fail(d, "unknown form " + std::to_string(s->form));
    if (s->n_total >= (1ull << 32)) return pod_fail(d, "2^32 entries or more");
    if (s->n_total & 1) return pod_fail(d, "n_total is odd");
    const uint64_t P = s->n_total / 2;
    if (s->form == PGRC_PAIRORDER_COMPLETE_SINGLE_FILE) {
        if (s->n_total && !s->rev) return pod_fail(d, "rev is absent (COMPLETE_SINGLE_FILE)");
        return PGRC_OK;
    }
    if (P && !s->off8_flag) return pod_fail(d, "off8_flag is NULL with a non-zero count");
    if (s->n_off8 && !s->off_value) return pod_fail(d, "off_value is NULL with a non-zero count");
    if (s->n_delta_flag && !s->delta8_flag) return pod_fail(d, "delta8_flag is NULL with a non-zero count");
    if (s->n_delta8 && !s->delta_value) return pod_fail(d, "delta_value is NULL with a non-zero count");
    if (s->n_full && !s->full_offset) return pod_fail(d, "full_offset is NULL with a non-zero count");
    if (s->form == PGRC_PAIRORDER_COMPLETE && P && !s->pair_base_org_idx) return pod_fail(d, "pair_base_org_idx is absent (COMPLETE)");
    if (s->form == PGRC_PAIRORDER_FILE_FLAGS && ((s->n_off8 && !s->off_base_file_flag) || (s->n_delta_flag && !s->nonoff_base_file_flag)))
        return pod_fail(d, "off_base_file_flag or nonoff_base_file_flag is absent (FILE_FLAGS)");
    // (counts beyond P cannot agree with the flags; refused here so that no buffer is sized by them)
    if (s->n_off8 > P || s->n_delta_flag > P || s->n_delta8 > P || s->n_full > P) return pod_fail(d, "a stream holds more elements than there are pairs");
    return PGRC_OK;
}

static std::string pod_findings(uint32_t f) {
    std::string m;
    if (f & POD_E_OFFSET) m += " a decoded offset below 1;";
    if (f & POD_E_MATE) m += " a mate beyond the last entry;";
    if (f & POD_E_PAIRS) m += " an entry that no pair takes (two pairs land on one entry);";
    if (f & POD_E_SLOTS) m += " the entries run out before the pairs do;";
    if (f & POD_E_ROUNDS) m += " internal: a word of the landing did not settle;";
    if (f & POD_E_PERM) m += " the landed pairs are not a permutation of the entries (two pairs land on one entry);";
    if (f & POD_E_PBO) m += " a pair_base_org_idx value of n_total or more;";
    m.pop_back();
    return m;
}

int pgrc_pairorder_decode_device(pgrc_decode_ctx *d, const pgrc_pairorder_streams *s, uint32_t *d_out) {
    PgrcPairOrderDec &st = d->pod;
    st.have_timing = false;
    const uint64_t T = s->n_total, P = T / 2;
    const int32_t form = s->form;
    const bool coded = form != PGRC_PAIRORDER_COMPLETE_SINGLE_FILE, ff = form == PGRC_PAIRORDER_FILE_FLAGS, complete = form == PGRC_PAIRORDER_COMPLETE;
    const uint64_t nf = coded ? s->n_delta_flag : 0;
    const auto t0 = std::chrono::steady_clock::now();
    int e;
    if ((e = st.ev.ensure(d))) return e;
    pgrc_pairorder_decode_timing t{};
    t.struct_size = sizeof(pgrc_pairorder_decode_timing);
    t.form = form;
    if (!coded) {
        if (T && (e = dec_upload_host(d, d_out, s->rev, T * 4))) return e;
        HIP_TRY(d, hipStreamSynchronize(d->stream));
        t.ms_upload = dec_ms_since(t0);
        t.bytes_up = T * 4;
        st.tm = t;
        return PGRC_OK;
    }
    const void *hsrc[PO_NS - 1] = {s->off8_flag, s->off_value, s->delta8_flag, s->delta_value, s->full_offset, s->pair_base_org_idx, s->off_base_file_flag, s->nonoff_base_file_flag};
    const uint64_t nbytes[PO_NS - 1] = {P, s->n_off8, nf, s->n_delta8, s->n_full * 4, complete ? P * 4 : 0, ff ? s->n_off8 : 0, ff ? nf : 0};
    const DecBlockLayout<PO_NS - 1> in = dec_block_layout(nbytes);
    const uint64_t ninc_at = 0, dinc_at = ninc_at + dec_a16(P * 4) + 16, d_at = dinc_at + dec_a16(nf * 4) + 16, pair_bytes = d_at + P * 4 + 16;
    const uint64_t nbatch = (T + POD_BATCH - 1) / POD_BATCH, map_bytes = std::max<uint64_t>(nbatch, 1) * POD_BATCH / 8;      // each bitmap: whole batches
    const uint64_t sco_bytes = dec_a16(sco_scratch_elems(P) * sizeof(PpSeg)), bsum_bytes = sco_bytes + 64;
    if ((e = pgrc_bufs_unpooled(d, {{&st.in, in.total}, {&st.pair, pair_bytes}, {&st.land, complete ? T * 4 + 16 : 16}, {&st.marks, 2 * map_bytes}, {&st.bsum, bsum_bytes}})))
        return e;
    uint8_t *ib = (uint8_t *)st.in.p, *pr = (uint8_t *)st.pair.p;
    for (int k = 0; k < PO_NS - 1; k++) {
        if (nbytes[k] && (e = dec_upload(d, ib + in.at[k], hsrc[k], nbytes[k]))) return e;
        t.bytes_up += nbytes[k];
    }
    t.ms_upload = dec_ms_since(t0);
    PoDecStreams ds;
    ds.off8_flag = ib + in.at[PO_OFF8];
    ds.off_val = ib + in.at[PO_OFFV];
    ds.del_flag = ib + in.at[PO_DELF];
    ds.del_val = (const int8_t *)(ib + in.at[PO_DELV]);
    ds.full = (const uint32_t *)(ib + in.at[PO_FULL]);
    uint32_t *near_inc = (uint32_t *)(pr + ninc_at), *del_inc = (uint32_t *)(pr + dinc_at), *dd = (uint32_t *)(pr + d_at);
    ds.near_inc = near_inc;
    ds.del_inc = del_inc;
    uint32_t *gmark = (uint32_t *)st.marks.p, *seen = (uint32_t *)((uint8_t *)st.marks.p + map_bytes);
    uint32_t *sco_tmp = (uint32_t *)st.bsum.p, *err = (uint32_t *)((uint8_t *)st.bsum.p + sco_bytes);      // err, -, count (u64), stat[2] (u64)
    unsigned long long *count = (unsigned long long *)(err + 2);
    uint64_t *stat = (uint64_t *)(err + 4);
    uint32_t *pe = complete ? (uint32_t *)st.land.p : d_out;

    // the flags' counts, held against the stream sizes before anything is indexed by them
    HIP_TRY(d, st.ev.record(0, d->stream));
    HIP_TRY(d, hipMemsetAsync(err, 0, 32, d->stream));
    HIP_TRY(d, sco_scan<true>(d->stream, ds.off8_flag, near_inc, P, PoNonZero{}, ScoPlus{}, 0u, sco_tmp));
    HIP_TRY(d, sco_scan<true>(d->stream, ds.del_flag, del_inc, nf, PoNonZero{}, ScoPlus{}, 0u, sco_tmp));
    uint32_t n_near = 0, n_del = 0;
    if (P) HIP_TRY(d, hipMemcpyAsync(&n_near, near_inc + P - 1, 4, hipMemcpyDeviceToHost, d->stream));
    if (nf) HIP_TRY(d, hipMemcpyAsync(&n_del, del_inc + nf - 1, 4, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    if (n_near != s->n_off8) return pod_fail(d, "off8_flag holds " + std::to_string(n_near) + " near pairs, n_off8 is " + std::to_string(s->n_off8));
    if (P - n_near != nf) return pod_fail(d, "off8_flag holds " + std::to_string(P - n_near) + " far pairs, n_delta_flag is " + std::to_string(nf));
    if (n_del != s->n_delta8) return pod_fail(d, "delta8_flag holds " + std::to_string(n_del) + " delta pairs, n_delta8 is " + std::to_string(s->n_delta8));
    if (nf - n_del != s->n_full) return pod_fail(d, "delta8_flag holds " + std::to_string(nf - n_del) + " full pairs, n_full is " + std::to_string(s->n_full));
    // refPrev at every pair; the scan's last pass writes every pair's offset
    HIP_TRY(d, st.ev.record(1, d->stream));     // (the host's wait above is no device time)
    HIP_TRY(d, (sco_device_scan<true, false>(d->stream, PoChainIn{ds}, P, PpSegOp{}, PpSeg{0, 0u}, PpSeg{0, 0u}, PoOffsetSink{ds, dd, err}, (PpSeg *)st.bsum.p)));
    HIP_TRY(d, st.ev.record(2, d->stream));
    HIP_TRY(d, hipMemsetAsync(gmark, 0, 2 * map_bytes, d->stream));
    if (P) hipLaunchKernelGGL(k_po_land, dim3(1), dim3(POD_TPB), 0, d->stream, (const uint32_t *)dd, P, pe, gmark, err, stat);
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, st.ev.record(3, d->stream));
    // the landing stops at its first finding and leaves the rest of pe as it was: nothing below runs on that
    uint32_t h_err[8] = {};
    HIP_TRY(d, hipMemcpyAsync(h_err, err, 32, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    if (h_err[0]) return pod_fail(d, pod_findings(h_err[0]));
    uint64_t h_stat[2];
    memcpy(h_stat, h_err + 4, 16);
    HIP_TRY(d, st.ev.record(6, d->stream));     // (the host's wait above is no device time)
    if (P) {
        hipLaunchKernelGGL(k_po_check, dim3(pp_grid(P)), dim3(PP_TPB), 0, d->stream, (const uint32_t *)pe, P, seen, err);
        hipLaunchKernelGGL(k_po_count, dim3(std::min(pp_grid(map_bytes / 4), 1024u)), dim3(PP_TPB), 0, d->stream, (const uint32_t *)seen, map_bytes / 4, count);
    }
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, st.ev.record(4, d->stream));
    if (P && ff) hipLaunchKernelGGL(k_po_tail_flags, dim3(pp_grid(P)), dim3(PP_TPB), 0, d->stream, P, ds.off8_flag, (const uint32_t *)near_inc, (const uint8_t *)(ib + in.at[PO_OFFF]),
                                    (const uint8_t *)(ib + in.at[PO_NONF]), d_out);
    if (P && complete) hipLaunchKernelGGL(k_po_tail_complete, dim3(pp_grid(P)), dim3(PP_TPB), 0, d->stream, P, (const uint32_t *)(ib + in.at[PO_PBO]), (const uint32_t *)pe, d_out, err);
    HIP_TRY(d, hipGetLastError());
    HIP_TRY(d, st.ev.record(5, d->stream));
    HIP_TRY(d, hipMemcpyAsync(h_err, err, 16, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    uint64_t h_count = 0;
    memcpy(&h_count, h_err + 2, 8);
    if (!h_err[0] && h_count != T) h_err[0] = POD_E_PERM;
    if (h_err[0]) return pod_fail(d, pod_findings(h_err[0]));
    t.ms_chain_device = st.ev.ms(0, 1) + st.ev.ms(1, 2);
    t.ms_landing_device = st.ev.ms(2, 3);
    t.ms_check_device = st.ev.ms(6, 4);
    t.ms_tail_device = st.ev.ms(4, 5);
    t.n_near = n_near;
    t.n_delta = n_del;
    t.n_full = nf - n_del;
    t.landing_words = h_stat[0];
    t.landing_rounds = h_stat[1];
    st.tm = t;
    return PGRC_OK;
}

extern "C" {

int pgrc_pairorder_decode(pgrc_decode_ctx *d, const pgrc_pairorder_streams *s, uint32_t *rl_idx_order) {
    if (!d) return PGRC_E_PARAM;
    int e;
    if ((e = pgrc_pairorder_check_streams(d, s))) return e;
    if (s->n_total && !rl_idx_order) return pod_fail(d, "rl_idx_order is NULL");
    PGRC_ON_DEVICE(d);
    const auto t0 = std::chrono::steady_clock::now();
    if ((e = pgrc_buf_unpooled(d, d->pod.out, s->n_total * 4 + 16))) return e;
    if ((e = pgrc_pairorder_decode_device(d, s, (uint32_t *)d->pod.out.p))) return e;
    const auto t1 = std::chrono::steady_clock::now();
    if ((e = dec_download_host(d, rl_idx_order, d->pod.out.p, s->n_total * 4))) return e;
    d->pod.tm.ms_download = dec_ms_since(t1);
    d->pod.tm.bytes_down = s->n_total * 4;
    d->pod.tm.ms_call = dec_ms_since(t0);
    d->pod.have_timing = true;
    return PGRC_OK;
}

int pgrc_pairorder_get_decode_timing(pgrc_decode_ctx *d, pgrc_pairorder_decode_timing *out) {
    if (!d) return PGRC_E_PARAM;
    if (!out || out->struct_size != sizeof(pgrc_pairorder_decode_timing)) return dec_fail(d, PGRC_E_PARAM, "timing is NULL or struct_size is not sizeof(pgrc_pairorder_decode_timing)");
    if (!d->pod.have_timing) return dec_fail(d, PGRC_E_STATE, "no pair-order decode has succeeded on this context");
    *out = d->pod.tm;
    return PGRC_OK;
}

int pgrc_pairorder_encode(pgrc_decode_ctx *d, const uint32_t *const org_idx[3], const uint64_t n[3], int32_t form, pgrc_pairorder_streams *out) {
    if (!d) return PGRC_E_PARAM;
    if (!out) return po_fail(d, "out is NULL");
    *out = pgrc_pairorder_streams{};
    if (!org_idx || !n) return po_fail(d, "org_idx or n is NULL");
    if (form < PGRC_PAIRORDER_IGNORE || form > PGRC_PAIRORDER_COMPLETE_SINGLE_FILE) return po_fail(d, "unknown form " + std::to_string(form));
    uint64_t T = 0;
    for (int l = 0; l < 3; l++) {
        if (n[l] >= (1ull << 32) || (T += n[l]) >= (1ull << 32)) return po_fail(d, "2^32 entries or more");
        if (n[l] && !org_idx[l]) return po_fail(d, "list " + std::to_string(l) + " is NULL with a non-zero count");
    }
    if (T & 1) return po_fail(d, "the entries' count is odd");
    PGRC_ON_DEVICE(d);
    d->po.have_timing = false;
    const int e = po_encode_run(d, d->po, org_idx, n, nullptr, T, form, out);
    if (e) *out = pgrc_pairorder_streams{};
    return e;
}

void pgrc_pairorder_free(pgrc_pairorder_streams *s) {
    if (!s) return;
    if (s->off8_flag) (void)hipHostFree(const_cast<uint8_t *>(s->off8_flag));
    *s = pgrc_pairorder_streams{};
}

int pgrc_pairorder_get_timing(pgrc_decode_ctx *d, pgrc_pairorder_timing *out) {
    if (!d) return PGRC_E_PARAM;
    if (!out || out->struct_size != sizeof(pgrc_pairorder_timing)) return dec_fail(d, PGRC_E_PARAM, "timing is NULL or struct_size is not sizeof(pgrc_pairorder_timing)");
    if (!d->po.have_timing) return dec_fail(d, PGRC_E_STATE, "no pair-order call has succeeded on this context");
    *out = d->po.tm;
    return PGRC_OK;
}

}   // extern "C"
