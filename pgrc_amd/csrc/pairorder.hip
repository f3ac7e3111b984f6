// pairorder.hip -- the pair-order coding of the paired mode that does not preserve the order, on the device: the encoder's
// SeparatedPseudoGenomePersistence::compressReadsOrder (SeparatedPseudoGenomePersistence.cpp:220-339; include/pgrc_decode.h,
// "The pair-order coding").
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

extern "C" {

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
