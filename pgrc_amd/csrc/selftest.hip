// selftest.hip -- test entries into the shared primitives: scanops.h's block scan and device scan, radix.hip's stable sort and
// segment sort; and into the hand-over: pack.hip's text and read kernels, mempack.hip's packing of a text that is in HBM already,
// what a context holds of its reads and its text after them, and stagectx.h's staged copies up and down.  Thin kernels and host wrappers, nothing else; linked with the product's objects into libpgrc_selftest.so
// (never into libpgrc_match.so).  tests/test_gpu_primitives.py, tests/test_gpu_handover.py, tests/test_gpu_memdev.py and
// tests/test_gpu_staging.py drive it against numpy; tests/test_gpu_verify.py reaches the verifier's pairing
// under keys of its own and the cut of its keys (verify.hip).
//
// Every entry takes host arrays (pgrc_selftest_mem_pack_device: its text at a device address), runs on the handle's device and returns host arrays.  Every device buffer that a primitive
// writes has a guard zone of ST_GUARD elements after its logical end, filled with ST_FILL bytes like the buffer itself; the
// entry reports in *guards which zones are still intact (one bit per zone).  The scan's fold scratch has exactly
// sco_scratch_elems(n) elements in front of its guard.
//
// Three preconditions of the primitives are met by construction and are not tested:
//   * the uint4 fast path of the u32 scan needs in.p aligned to 16 bytes (the buffers come straight from hipMalloc);
//   * k_pack_ascii's 16-byte loads need its ASCII input aligned to 16 bytes (pgrc_selftest_pack_text: straight from hipMalloc,
//     as the product's staging buffer is);
//   * sco_block_exclusive<NWV = 0> needs blockDim.x to be a multiple of 64 (the entry refuses anything else).
#include <vector>

#include "ctx.h"
#include "scanops.h"
#include "stagectx.h"
#include "verifyctx.h"

#define ST_GUARD 64
#define ST_FILL 0xA5

struct pgrc_selftest {
    PgrcDev dev;                        // with a stream of its own
    DevBuf sort_scratch;
};

namespace {

struct StBuf {                          // `bytes` logical bytes and `guard` bytes after them, all ST_FILL at first
                                        // (and 16 spare bytes behind the guard, unchecked: an empty buffer without a guard, the
                                        // input of n = 0, is still a real allocation)
    uint8_t *p = nullptr;
    size_t bytes = 0, guard = 0;
    ~StBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t logical, size_t guard_bytes) {
        bytes = logical;
        guard = guard_bytes;
        hipError_t e = hipMalloc((void **)&p, bytes + guard + 16);
        if (e != hipSuccess) return e;
        return hipMemset(p, ST_FILL, bytes + guard + 16);
    }
    hipError_t intact(bool *ok) const {
        std::vector<uint8_t> h(guard);
        hipError_t e = hipMemcpy(h.data(), p + bytes, guard, hipMemcpyDeviceToHost);
        *ok = true;
        for (uint8_t b : h) *ok &= b == ST_FILL;
        return e;
    }
};

// the operators of the library's scans, restated (their originals live in mem.hip, pgmap.hip and pairpos.hip)
struct StIsOne { __device__ uint32_t operator()(uint8_t x) const { return x == 1u ? 1u : 0u; } };
struct StMax { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; } };
#define ST_NONE 0xFFFFFFFFu
struct StLastValid { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return b != ST_NONE ? b : a; } };
struct __attribute__((packed, aligned(4))) StSeg {      // 12 bytes: three words to shuffle
    int64_t v;
    uint32_t set;
};
struct StSegOp { __device__ StSeg operator()(StSeg a, StSeg b) const { return b.set ? b : StSeg{a.v + b.v, a.set}; } };

enum {
    ST_U32_SUM_U32 = 0,     // sco_scan, identity transform (uint4 loads on whole blocks)
    ST_U32_FLAG_U8 = 1,     // sco_scan through a predicate
    ST_U64_SUM_U8 = 2,      // sco_sum_u64 (start = 0, total) / sco_device_scan with start
    ST_U64_SUM_U16 = 3,
    ST_U64_SUM_U32 = 4,
    ST_U64_SUM_U64 = 5,
    ST_U64_MAX = 6,
    ST_U32_LAST_VALID = 7,  // non-commuting, identity ST_NONE
    ST_SEG_SUM = 8,         // the 12-byte (int64, set) element
    ST_KINDS = 9
};
const size_t k_in_size[ST_KINDS] = {4, 1, 1, 2, 4, 8, 8, 4, 12}, k_t_size[ST_KINDS] = {4, 4, 8, 8, 8, 8, 8, 4, 12};

template <typename In>
hipError_t st_sum_u64(hipStream_t s, const void *in, uint64_t n, uint64_t start, bool inclusive, bool total, uint64_t *out, uint64_t *fold) {
    const In *p = (const In *)in;
    if (total && !start) return inclusive ? sco_sum_u64<true>(s, p, n, out, fold) : sco_sum_u64<false>(s, p, n, out, fold);
    const ScoLoad<uint64_t, In, ScoIdentity> ld{p, ScoIdentity{}};
    const ScoStore<uint64_t> st{out};
    if (total)
        return inclusive ? sco_device_scan<true, true>(s, ld, n, ScoPlus{}, (uint64_t)0, start, st, fold)
                         : sco_device_scan<false, true>(s, ld, n, ScoPlus{}, (uint64_t)0, start, st, fold);
    return inclusive ? sco_device_scan<true, false>(s, ld, n, ScoPlus{}, (uint64_t)0, start, st, fold)
                     : sco_device_scan<false, false>(s, ld, n, ScoPlus{}, (uint64_t)0, start, st, fold);
}

template <typename In, typename Xf, typename Op>
hipError_t st_scan_u32(hipStream_t s, const void *in, void *out, uint64_t n, bool inclusive, Xf xf, Op op, uint32_t ident, void *fold) {
    return inclusive ? sco_scan<true>(s, (const In *)in, (uint32_t *)out, n, xf, op, ident, (uint32_t *)fold)
                     : sco_scan<false>(s, (const In *)in, (uint32_t *)out, n, xf, op, ident, (uint32_t *)fold);
}

template <typename T, typename Op>
hipError_t st_scan_plain(hipStream_t s, const void *in, void *out, uint64_t n, bool inclusive, Op op, T ident, void *fold) {
    const ScoLoad<T, T, ScoIdentity> ld{(const T *)in, ScoIdentity{}};
    const ScoStore<T> st{(T *)out};
    return inclusive ? sco_device_scan<true, false>(s, ld, n, op, ident, ident, st, (T *)fold)
                     : sco_device_scan<false, false>(s, ld, n, op, ident, ident, st, (T *)fold);
}

// one block: every thread's exclusive value and the total it was handed; then a second scan over the same smem, of
// op(first exclusive value, the input in reverse thread order)
template <int NWV, bool SYNC, typename T, typename Op>
__global__ void __launch_bounds__(1024) k_st_block(const T *__restrict__ in, Op op, T ident, T *__restrict__ ex, T *__restrict__ tot, T *__restrict__ second) {
    __shared__ T smem[16];
    const uint32_t t = threadIdx.x;
    T total, total2;
    const T e = sco_block_exclusive<NWV, SYNC>(in[t], op, ident, smem, &total);
    ex[t] = e;
    tot[t] = total;
    if (!SYNC) __syncthreads();
    const T v2 = op(e, in[blockDim.x - 1u - t]);
    second[t] = sco_block_exclusive<NWV, SYNC>(v2, op, ident, smem, &total2);
}

template <typename T, typename Op>
int st_block_run(pgrc_selftest *h, uint32_t threads, bool nwv_static, bool sync_after, const void *in, Op op, T ident, void *ex, void *tot, void *second,
                 uint32_t *guards) {
    PgrcDev *c = &h->dev;
    const size_t bytes = (size_t)threads * sizeof(T);
    StBuf din, dout[3];
    HIP_TRY(c, din.alloc(bytes, 0));
    for (StBuf &b : dout) HIP_TRY(c, b.alloc(bytes, ST_GUARD * sizeof(T)));
    HIP_TRY(c, hipMemcpy(din.p, in, bytes, hipMemcpyHostToDevice));
#define ST_LAUNCH(NWV, SYNC)                                                                                                              \
    hipLaunchKernelGGL((k_st_block<NWV, SYNC, T, Op>), dim3(1), dim3(threads), 0, c->stream, (const T *)din.p, op, ident, (T *)dout[0].p, \
                       (T *)dout[1].p, (T *)dout[2].p)
#define ST_CASE(NWV)                 \
    case NWV:                        \
        if (sync_after) {            \
            ST_LAUNCH(NWV, true);    \
        } else {                     \
            ST_LAUNCH(NWV, false);   \
        }                            \
        break;
    switch (nwv_static ? threads / 64u : 0u) {
        ST_CASE(0)
        ST_CASE(1)
        ST_CASE(2)
        ST_CASE(4)
        ST_CASE(8)
        ST_CASE(16)
    default:
        c->err = "selftest: no block scan for this block size";
        return PGRC_E_PARAM;
    }
#undef ST_CASE
#undef ST_LAUNCH
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    void *host[3] = {ex, tot, second};
    *guards = 0;
    for (int k = 0; k < 3; k++) {
        bool ok;
        HIP_TRY(c, hipMemcpy(host[k], dout[k].p, bytes, hipMemcpyDeviceToHost));
        HIP_TRY(c, dout[k].intact(&ok));
        *guards |= (ok ? 1u : 0u) << k;
    }
    return PGRC_OK;
}

}  // namespace

extern "C" int pgrc_selftest_create(int device, pgrc_selftest **out) {
    *out = nullptr;
    pgrc_selftest *h = new pgrc_selftest();
    h->dev.device = device;
    PgrcDeviceScope scope(device);
    if (!scope.ok || hipStreamCreate(&h->dev.stream) != hipSuccess) {
        delete h;
        return PGRC_E_NO_DEVICE;
    }
    *out = h;
    return PGRC_OK;
}

extern "C" void pgrc_selftest_destroy(pgrc_selftest *h) {
    if (!h) return;
    PgrcDeviceScope scope(h->dev.device);
    (void)hipStreamSynchronize(h->dev.stream);
    pgrc_buf_free(h->sort_scratch);
    (void)hipStreamDestroy(h->dev.stream);
    delete h;
}

extern "C" const char *pgrc_selftest_last_error(const pgrc_selftest *h) { return h->dev.err.c_str(); }

extern "C" uint64_t pgrc_selftest_scratch_elems(uint64_t n) { return sco_scratch_elems(n); }

// out: n + 1 elements of the kind's output type (element n is ST_FILL bytes unless the scan wrote a total there).
// *guards: bit 0 the zone after out[n], bit 1 the zone after the fold scratch.  in_place: the scan reads what it writes (kinds
// whose input and output elements have one size).  start and total_at_n: the u64 sums only.
extern "C" int pgrc_selftest_device_scan(pgrc_selftest *h, int kind, const void *in, uint64_t n, uint64_t start, int inclusive, int total_at_n, int in_place,
                                         void *out, uint32_t *guards) {
    PgrcDev *c = &h->dev;
    PGRC_ON_DEVICE(c);
    const bool u64sum = kind >= ST_U64_SUM_U8 && kind <= ST_U64_SUM_U64;
    if (kind < 0 || kind >= ST_KINDS || (!u64sum && (start || total_at_n)) || (in_place && k_in_size[kind] != k_t_size[kind])) {
        c->err = "selftest: no such scan";
        return PGRC_E_PARAM;
    }
    const size_t isz = k_in_size[kind], tsz = k_t_size[kind];
    StBuf din, dout, dfold;
    HIP_TRY(c, dout.alloc((n + 1) * tsz, ST_GUARD * tsz));
    HIP_TRY(c, dfold.alloc(sco_scratch_elems(n) * tsz, ST_GUARD * tsz));
    if (!in_place) HIP_TRY(c, din.alloc(n * isz, 0));
    const void *src = in_place ? dout.p : din.p;
    if (n) HIP_TRY(c, hipMemcpy((void *)src, in, n * isz, hipMemcpyHostToDevice));
    hipStream_t s = c->stream;
    const bool inc = inclusive != 0;
    hipError_t e = hipSuccess;
    switch (kind) {
    case ST_U32_SUM_U32: e = st_scan_u32<uint32_t>(s, src, dout.p, n, inc, ScoIdentity{}, ScoPlus{}, 0u, dfold.p); break;
    case ST_U32_FLAG_U8: e = st_scan_u32<uint8_t>(s, src, dout.p, n, inc, StIsOne{}, ScoPlus{}, 0u, dfold.p); break;
    case ST_U64_SUM_U8: e = st_sum_u64<uint8_t>(s, src, n, start, inc, total_at_n != 0, (uint64_t *)dout.p, (uint64_t *)dfold.p); break;
    case ST_U64_SUM_U16: e = st_sum_u64<uint16_t>(s, src, n, start, inc, total_at_n != 0, (uint64_t *)dout.p, (uint64_t *)dfold.p); break;
    case ST_U64_SUM_U32: e = st_sum_u64<uint32_t>(s, src, n, start, inc, total_at_n != 0, (uint64_t *)dout.p, (uint64_t *)dfold.p); break;
    case ST_U64_SUM_U64: e = st_sum_u64<uint64_t>(s, src, n, start, inc, total_at_n != 0, (uint64_t *)dout.p, (uint64_t *)dfold.p); break;
    case ST_U64_MAX: e = st_scan_plain<uint64_t>(s, src, dout.p, n, inc, StMax{}, (uint64_t)0, dfold.p); break;
    case ST_U32_LAST_VALID: e = st_scan_u32<uint32_t>(s, src, dout.p, n, inc, ScoIdentity{}, StLastValid{}, ST_NONE, dfold.p); break;
    case ST_SEG_SUM: e = st_scan_plain<StSeg>(s, src, dout.p, n, inc, StSegOp{}, StSeg{0, 0u}, dfold.p); break;
    }
    HIP_TRY(c, e);
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipMemcpy(out, dout.p, (n + 1) * tsz, hipMemcpyDeviceToHost));
    bool ok_out, ok_fold;
    HIP_TRY(c, dout.intact(&ok_out));
    HIP_TRY(c, dfold.intact(&ok_fold));
    *guards = (ok_out ? 1u : 0u) | (ok_fold ? 2u : 0u);
    return PGRC_OK;
}

// One block of block_threads threads (a multiple of 64, at most 1024).  kind: 0 sum over u32, 1 sum over u64, 2 maximum over
// u64, 3 the 12-byte segmented sum.  nwv_static: the wave count as a template argument, else NWV = 0.  With sync_after = 0 the
// kernel puts its own barrier between the two scans.  *guards: bits 0..2, the zones after the three outputs.
extern "C" int pgrc_selftest_block_scan(pgrc_selftest *h, int kind, uint32_t block_threads, int nwv_static, int sync_after, const void *in, void *out_exclusive,
                                        void *out_total_per_thread, void *out_second, uint32_t *guards) {
    PgrcDev *c = &h->dev;
    PGRC_ON_DEVICE(c);
    if (!block_threads || block_threads % 64u || block_threads > 1024u) {
        c->err = "selftest: the block scan needs whole waves, at most 16";
        return PGRC_E_PARAM;
    }
    const bool st = nwv_static != 0, sy = sync_after != 0;
    switch (kind) {
    case 0: return st_block_run<uint32_t>(h, block_threads, st, sy, in, ScoPlus{}, 0u, out_exclusive, out_total_per_thread, out_second, guards);
    case 1: return st_block_run<uint64_t>(h, block_threads, st, sy, in, ScoPlus{}, (uint64_t)0, out_exclusive, out_total_per_thread, out_second, guards);
    case 2: return st_block_run<uint64_t>(h, block_threads, st, sy, in, StMax{}, (uint64_t)0, out_exclusive, out_total_per_thread, out_second, guards);
    case 3: return st_block_run<StSeg>(h, block_threads, st, sy, in, StSegOp{}, StSeg{0, 0u}, out_exclusive, out_total_per_thread, out_second, guards);
    }
    c->err = "selftest: no such block scan";
    return PGRC_E_PARAM;
}

// pgrc_radix_sort_u64 (vals = null) or pgrc_radix_sort_pairs_u64, copied from wherever *sorted points.  *guards: bits 0, 1 the
// zones after the two key buffers, bits 2, 3 after the two value buffers (set when there are none).
extern "C" int pgrc_selftest_sort(pgrc_selftest *h, const uint64_t *keys, const uint64_t *vals, uint64_t n, uint32_t bit_lo, uint32_t bit_hi, uint64_t *out_keys,
                                  uint64_t *out_vals, uint32_t *guards) {
    PgrcDev *c = &h->dev;
    PGRC_ON_DEVICE(c);
    StBuf k[2], v[2];
    for (StBuf &b : k) HIP_TRY(c, b.alloc(n * 8, ST_GUARD * 8));
    if (n) HIP_TRY(c, hipMemcpy(k[0].p, keys, n * 8, hipMemcpyHostToDevice));
    uint64_t *ks = nullptr, *vs = nullptr;
    int e;
    if (vals) {
        for (StBuf &b : v) HIP_TRY(c, b.alloc(n * 8, ST_GUARD * 8));
        if (n) HIP_TRY(c, hipMemcpy(v[0].p, vals, n * 8, hipMemcpyHostToDevice));
        e = pgrc_radix_sort_pairs_u64(c, (uint64_t *)k[0].p, (uint64_t *)k[1].p, (uint64_t *)v[0].p, (uint64_t *)v[1].p, n, bit_lo, bit_hi, h->sort_scratch, &ks, &vs);
    } else {
        e = pgrc_radix_sort_u64(c, (uint64_t *)k[0].p, (uint64_t *)k[1].p, n, bit_lo, bit_hi, h->sort_scratch, &ks);
    }
    if (e) return e;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n) HIP_TRY(c, hipMemcpy(out_keys, ks, n * 8, hipMemcpyDeviceToHost));
    if (n && vals) HIP_TRY(c, hipMemcpy(out_vals, vs, n * 8, hipMemcpyDeviceToHost));
    *guards = vals ? 0u : 12u;
    for (int i = 0; i < 2; i++) {
        bool ok;
        HIP_TRY(c, k[i].intact(&ok));
        *guards |= (ok ? 1u : 0u) << i;
        if (vals) {
            HIP_TRY(c, v[i].intact(&ok));
            *guards |= (ok ? 4u : 0u) << i;
        }
    }
    return PGRC_OK;
}

// pgrc_radix_sort_segments_pairs_u64 over seg[0 .. nseg] (seg[nseg] pairs in all), in place.  out_ovl: cap + 1 words, the words
// the kernel did not write are ST_FILL bytes.  *guards: bits 0, 1 the zones after keys and values, bit 2 after ovl[cap].
extern "C" int pgrc_selftest_sort_segments(pgrc_selftest *h, const uint64_t *keys, const uint64_t *vals, const uint32_t *seg, uint32_t nseg, uint32_t bit_lo,
                                           uint32_t bit_hi, uint32_t top_bits, uint32_t cap, uint64_t *out_keys, uint64_t *out_vals, uint32_t *out_ovl,
                                           uint32_t *guards) {
    PgrcDev *c = &h->dev;
    PGRC_ON_DEVICE(c);
    const uint64_t n = seg[nseg];
    StBuf k, v, ds, ovl;
    HIP_TRY(c, k.alloc(n * 8, ST_GUARD * 8));
    HIP_TRY(c, v.alloc(n * 8, ST_GUARD * 8));
    HIP_TRY(c, ds.alloc(((size_t)nseg + 1) * 4, 0));
    HIP_TRY(c, ovl.alloc(((size_t)cap + 1) * 4, ST_GUARD * 4));
    if (n) {
        HIP_TRY(c, hipMemcpy(k.p, keys, n * 8, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(v.p, vals, n * 8, hipMemcpyHostToDevice));
    }
    HIP_TRY(c, hipMemcpy(ds.p, seg, ((size_t)nseg + 1) * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemset(ovl.p, 0, 4));
    const int e = pgrc_radix_sort_segments_pairs_u64(c, (uint64_t *)k.p, (uint64_t *)v.p, (const uint32_t *)ds.p, nseg, bit_lo, bit_hi, (uint32_t *)ovl.p, cap, top_bits);
    if (e) return e;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n) {
        HIP_TRY(c, hipMemcpy(out_keys, k.p, n * 8, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(out_vals, v.p, n * 8, hipMemcpyDeviceToHost));
    }
    HIP_TRY(c, hipMemcpy(out_ovl, ovl.p, ((size_t)cap + 1) * 4, hipMemcpyDeviceToHost));
    bool ok[3];
    HIP_TRY(c, k.intact(&ok[0]));
    HIP_TRY(c, v.intact(&ok[1]));
    HIP_TRY(c, ovl.intact(&ok[2]));
    *guards = (ok[0] ? 1u : 0u) | (ok[1] ? 2u : 0u) | (ok[2] ? 4u : 0u);
    return PGRC_OK;
}

// ------------------------------------------------------------------ the hand-over (pack.hip; tests/test_gpu_handover.py)

// pgrc_launch_pack_ascii over `count` >= 1 host symbols.  out_words: ceil(count / 16) words.  *guards: bit 0 the zone after the
// words, bit 1 the zone after the error flag.
extern "C" int pgrc_selftest_pack_text(pgrc_selftest *h, const uint8_t *ascii, uint64_t count, uint32_t *out_words, uint32_t *out_err, uint32_t *guards) {
    PgrcDev *c = &h->dev;
    PGRC_ON_DEVICE(c);
    if (!count) {
        c->err = "selftest: an empty text launches nothing";
        return PGRC_E_PARAM;
    }
    const uint64_t nwords = (count + 15) / 16;
    StBuf din, dw, dflag;
    HIP_TRY(c, din.alloc(count, 0));
    HIP_TRY(c, dw.alloc(nwords * 4, ST_GUARD * 4));
    HIP_TRY(c, dflag.alloc(4, ST_GUARD * 4));
    HIP_TRY(c, hipMemcpy(din.p, ascii, count, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemset(dflag.p, 0, 4));
    const int e = pgrc_launch_pack_ascii(c, c->stream, din.p, count, (uint32_t *)dw.p, (uint32_t *)dflag.p);
    if (e) return e;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out_words, dw.p, nwords * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(out_err, dflag.p, 4, hipMemcpyDeviceToHost));
    bool ok_w, ok_f;
    HIP_TRY(c, dw.intact(&ok_w));
    HIP_TRY(c, dflag.intact(&ok_f));
    *guards = (ok_w ? 1u : 0u) | (ok_f ? 2u : 0u);
    return PGRC_OK;
}

// pgrc_launch_mem_pack_device (mempack.hip; tests/test_gpu_memdev.py) over the n >= 1 ASCII bytes at the DEVICE address d_ascii,
// which may have any alignment, forward or reverse-complemented, in at most block_cap blocks (0: no cap of the entry's own; a
// small cap makes a short text loop in the grid stride).  As the matcher asks for it: ceil(n / 16) + PGRC_PG_PAD_WORDS words
// and as many 16-bit N masks (with_nmap = 0: none, out_nmap comes back as ST_FILL bytes), all pre-filled with ST_FILL; the flag
// word starts as zero.  *guards: bit 0 the zone after the words, bit 1 after the N map, bit 2 after the flag word.
extern "C" int pgrc_selftest_mem_pack_device(pgrc_selftest *h, const void *d_ascii, uint64_t n, int reversed, uint32_t block_cap, int with_nmap,
                                             uint32_t *out_words, uint16_t *out_nmap, uint32_t *out_flags, uint32_t *guards) {
    PgrcDev *c = &h->dev;
    PGRC_ON_DEVICE(c);
    if (!n || !d_ascii) {
        c->err = "selftest: an empty text launches nothing";
        return PGRC_E_PARAM;
    }
    const uint64_t total = (n + 15) / 16 + PGRC_PG_PAD_WORDS;
    StBuf dw, dn, dflag;
    HIP_TRY(c, dw.alloc(total * 4, ST_GUARD * 4));
    HIP_TRY(c, dn.alloc(total * 2, ST_GUARD * 2));
    HIP_TRY(c, dflag.alloc(4, ST_GUARD * 4));
    HIP_TRY(c, hipMemset(dflag.p, 0, 4));
    HIP_TRY(c, hipDeviceSynchronize());          // (the caller's text may have been written on another stream)
    const int e = pgrc_launch_mem_pack_device(c, (const uint8_t *)d_ascii, n, reversed != 0, (uint32_t *)dw.p, with_nmap ? (uint16_t *)dn.p : nullptr, total,
                                              (uint32_t *)dflag.p, block_cap);
    if (e) return e;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out_words, dw.p, total * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(out_nmap, dn.p, total * 2, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(out_flags, dflag.p, 4, hipMemcpyDeviceToHost));
    const StBuf *zone[3] = {&dw, &dn, &dflag};
    *guards = 0;
    for (int k = 0; k < 3; k++) {
        bool ok;
        HIP_TRY(c, zone[k]->intact(&ok));
        *guards |= (ok ? 1u : 0u) << k;
    }
    return PGRC_OK;
}

// The same launch `repeats` times into buffers made once, HIP events around each: ms[0 .. repeats) is the kernel's device time
// (tools/mem_resident_rate.py sets it beside a device-to-device copy of the text's bytes).  No guard zones, nothing comes back.
extern "C" int pgrc_selftest_mem_pack_time(pgrc_selftest *h, const void *d_ascii, uint64_t n, int reversed, uint32_t repeats, float *ms) {
    PgrcDev *c = &h->dev;
    PGRC_ON_DEVICE(c);
    if (!n || !d_ascii || !ms) {
        c->err = "selftest: an empty text launches nothing";
        return PGRC_E_PARAM;
    }
    const uint64_t total = (n + 15) / 16 + PGRC_PG_PAD_WORDS;
    StBuf dw, dn, dflag;
    HIP_TRY(c, dw.alloc(total * 4, 0));
    HIP_TRY(c, dn.alloc(total * 2, 0));
    HIP_TRY(c, dflag.alloc(4, 0));
    hipEvent_t ev[2];
    HIP_TRY(c, hipEventCreate(&ev[0]));
    HIP_TRY(c, hipEventCreate(&ev[1]));
    HIP_TRY(c, hipDeviceSynchronize());
    int e = PGRC_OK;
    for (uint32_t r = 0; r < repeats && !e; r++) {
        (void)hipEventRecord(ev[0], c->stream);
        e = pgrc_launch_mem_pack_device(c, (const uint8_t *)d_ascii, n, reversed != 0, (uint32_t *)dw.p, (uint16_t *)dn.p, total, (uint32_t *)dflag.p, 0);
        (void)hipEventRecord(ev[1], c->stream);
        if (!e && (hipEventSynchronize(ev[1]) != hipSuccess || hipEventElapsedTime(&ms[r], ev[0], ev[1]) != hipSuccess)) {
            c->err = "selftest: timing the packing kernel failed";
            e = PGRC_E_DEVICE;
        }
    }
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    return e;
}

// pgrc_launch_revcomp over ceil(G / 16) host words, G >= 1.  The forward buffer carries PGRC_PG_PAD_WORDS zero words behind the
// text, as pgrc_pg_alloc provides (the kernel reads fw[q + 1]).  *guards: bit 0 the zone after the output words.
extern "C" int pgrc_selftest_revcomp(pgrc_selftest *h, const uint32_t *words, uint64_t G, uint32_t *out_words, uint32_t *guards) {
    PgrcDev *c = &h->dev;
    PGRC_ON_DEVICE(c);
    if (!G) {
        c->err = "selftest: an empty text launches nothing";
        return PGRC_E_PARAM;
    }
    const uint64_t nwords = (G + 15) / 16;
    StBuf dfw, drc;
    HIP_TRY(c, dfw.alloc((nwords + PGRC_PG_PAD_WORDS) * 4, 0));
    HIP_TRY(c, drc.alloc(nwords * 4, ST_GUARD * 4));
    HIP_TRY(c, hipMemset(dfw.p, 0, (nwords + PGRC_PG_PAD_WORDS) * 4));
    HIP_TRY(c, hipMemcpy(dfw.p, words, nwords * 4, hipMemcpyHostToDevice));
    const int e = pgrc_launch_revcomp(c, c->stream, (const uint32_t *)dfw.p, (uint32_t *)drc.p, G);
    if (e) return e;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out_words, drc.p, nwords * 4, hipMemcpyDeviceToHost));
    bool ok;
    HIP_TRY(c, drc.intact(&ok));
    *guards = ok ? 1u : 0u;
    return PGRC_OK;
}

// One block of `count` rows put at reads [first, first + count) of a set of n_total reads: kind 0 ASCII rows
// (k_pack_reads_ascii), 4 the reference's ACGT packing (k_repack_reads_ref), 5 its ACGNT packing (k_unpack_reads_acgnt); then
// k_npos_rows for kinds 0 and 5 -- the sequence of append_rows (api.hip).  The word array of ceil(L / 16) * stride words and
// npos[n_total] start as ST_FILL bytes, nflag[n_total] as zeros (begin_reads clears it); all three come back whole.
// *guards: bit 0 the zone after the words, 1 after nflag, 2 after npos, 3 after the error flag.
extern "C" int pgrc_selftest_pack_reads(pgrc_selftest *h, int kind, const uint8_t *rows, uint64_t first, uint64_t count, uint32_t L, uint64_t n_total,
                                        uint64_t stride, uint32_t *out_words, uint8_t *out_nflag, uint32_t *out_npos, uint32_t *out_err, uint32_t *guards) {
    PgrcDev *c = &h->dev;
    PGRC_ON_DEVICE(c);
    if ((kind != 0 && kind != 4 && kind != 5) || !L || L > 255 || !count || first + count > n_total || n_total > stride) {
        c->err = "selftest: no such block of reads";
        return PGRC_E_PARAM;
    }
    const uint32_t nw = (L + 15) / 16, rb = kind == 0 ? L : kind == 4 ? (L + 3) / 4 : (L + 2) / 3;
    StBuf drows, dw, dnf, dnp, dflag;
    HIP_TRY(c, drows.alloc(count * rb, 0));
    HIP_TRY(c, dw.alloc((size_t)nw * stride * 4, ST_GUARD * 4));
    HIP_TRY(c, dnf.alloc(n_total, ST_GUARD));
    HIP_TRY(c, dnp.alloc(n_total * 4, ST_GUARD * 4));
    HIP_TRY(c, dflag.alloc(4, ST_GUARD * 4));
    HIP_TRY(c, hipMemcpy(drows.p, rows, count * rb, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemset(dnf.p, 0, n_total));
    HIP_TRY(c, hipMemset(dflag.p, 0, 4));
    int e;
    if (kind == 0) e = pgrc_launch_pack_reads_ascii(c, c->stream, drows.p, first, count, L, (uint32_t *)dw.p, stride, dnf.p, (uint32_t *)dflag.p);
    else if (kind == 4) e = pgrc_launch_repack_reads_ref(c, c->stream, drows.p, first, count, L, (uint32_t *)dw.p, stride);
    else e = pgrc_launch_unpack_reads_acgnt(c, c->stream, drows.p, first, count, L, (uint32_t *)dw.p, stride, dnf.p, (uint32_t *)dflag.p);
    if (!e && kind != 4) e = pgrc_launch_npos_rows(c, c->stream, drows.p, kind, first, count, L, dnf.p, (uint32_t *)dnp.p);
    if (e) return e;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out_words, dw.p, (size_t)nw * stride * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(out_nflag, dnf.p, n_total, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(out_npos, dnp.p, n_total * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(out_err, dflag.p, 4, hipMemcpyDeviceToHost));
    const StBuf *zone[4] = {&dw, &dnf, &dnp, &dflag};
    *guards = 0;
    for (int k = 0; k < 4; k++) {
        bool ok;
        HIP_TRY(c, zone[k]->intact(&ok));
        *guards |= (ok ? 1u : 0u) << k;
    }
    return PGRC_OK;
}

// pgrc_launch_nrows_ascii_acgnt: the ASCII rows of the ACGNT-packed rows local_idx[0 .. count) (each below n_rows), in that
// order.  *guards: bit 0 the zone after the count * L output bytes.
extern "C" int pgrc_selftest_nrows_ascii(pgrc_selftest *h, const uint8_t *packed, uint64_t n_rows, const uint32_t *local_idx, uint64_t count, uint32_t L,
                                         uint8_t *out_ascii, uint32_t *guards) {
    PgrcDev *c = &h->dev;
    PGRC_ON_DEVICE(c);
    bool inside = L && L <= 255 && count;
    for (uint64_t k = 0; inside && k < count; k++) inside = local_idx[k] < n_rows;
    if (!inside) {
        c->err = "selftest: no such rows";
        return PGRC_E_PARAM;
    }
    const uint32_t pb = (L + 2) / 3;
    StBuf drows, didx, dout;
    HIP_TRY(c, drows.alloc(n_rows * pb, 0));
    HIP_TRY(c, didx.alloc(count * 4, 0));
    HIP_TRY(c, dout.alloc(count * L, ST_GUARD));
    HIP_TRY(c, hipMemcpy(drows.p, packed, n_rows * pb, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(didx.p, local_idx, count * 4, hipMemcpyHostToDevice));
    const int e = pgrc_launch_nrows_ascii_acgnt(c, c->stream, drows.p, (const uint32_t *)didx.p, count, L, dout.p);
    if (e) return e;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out_ascii, dout.p, count * L, hipMemcpyDeviceToHost));
    bool ok;
    HIP_TRY(c, dout.intact(&ok));
    *guards = ok ? 1u : 0u;
    return PGRC_OK;
}

// What a context of the PRODUCT library holds after a hand-over, read only.  libpgrc_match.so and this library are linked from
// the same objects in one `make`, so pgrc_match_ctx and pgrc_multi have one layout in both; this library's copy of
// pgrc_multi_shards reads the front's shard list.  shard < 0: `ctx` is a single-device context; otherwise shard `shard` of the
// multi-device front `ctx`.  info[0 .. 10): n, stride, nw, n_nreads, n_many, 1 where nread_npos was ever allocated, pg_words,
// the shard's first read, its end, the number of shards.  Every output may be null (a first call asks for info alone):
// reads2 nw * stride words, nflag n bytes, npos n words, nidx n_nreads words, nascii n_nreads * read_len bytes, text pg_words
// words of the forward text.
extern "C" int pgrc_selftest_reads_state(pgrc_selftest *h, const pgrc_match_ctx *ctx, int32_t shard, uint64_t *info, uint32_t *out_reads2, uint8_t *out_nflag,
                                         uint32_t *out_npos, uint32_t *out_nidx, uint8_t *out_nascii, uint32_t *out_text) {
    PgrcDev *c = &h->dev;
    if (!ctx || !info || (shard < 0) != (ctx->multi == nullptr)) {
        c->err = "selftest: no such context or shard";
        return PGRC_E_PARAM;
    }
    const pgrc_match_ctx *s = ctx;
    uint64_t lo = 0, hi = ctx->rd.n, shards = 1;
    if (ctx->multi) {
        const std::vector<PgrcShardView> v = pgrc_multi_shards(const_cast<pgrc_match_ctx *>(ctx));
        if ((size_t)shard >= v.size()) {
            c->err = "selftest: no such context or shard";
            return PGRC_E_PARAM;
        }
        s = v[shard].ctx;
        lo = v[shard].lo;
        hi = v[shard].hi;
        shards = v.size();
    }
    const bool has_npos = s->rd.nread_npos.p && s->rd.nread_npos.bytes >= s->rd.n * 4;
    const uint64_t vals[10] = {s->rd.n, s->rd.stride, s->rd.nw, s->rd.n_nreads, s->rd.n_many, has_npos ? 1u : 0u, s->txt.have_pg ? s->txt.pg_words : 0, lo, hi, shards};
    for (int k = 0; k < 10; k++) info[k] = vals[k];
    PgrcDeviceScope scope(s->device);
    if (!scope.ok) {
        c->err = "selftest: hipSetDevice failed";
        return PGRC_E_NO_DEVICE;
    }
    HIP_TRY(c, hipDeviceSynchronize());
    if (out_reads2 && s->rd.have_reads && s->rd.n) HIP_TRY(c, hipMemcpy(out_reads2, s->rd.reads2, (size_t)s->rd.nw * s->rd.stride * 4, hipMemcpyDeviceToHost));
    if (out_nflag && s->rd.n && s->rd.nread_flag.p) HIP_TRY(c, hipMemcpy(out_nflag, s->rd.nread_flag.p, s->rd.n, hipMemcpyDeviceToHost));
    if (out_npos && s->rd.n && has_npos) HIP_TRY(c, hipMemcpy(out_npos, s->rd.nread_npos.p, s->rd.n * 4, hipMemcpyDeviceToHost));
    if (out_nidx && s->rd.n_nreads) HIP_TRY(c, hipMemcpy(out_nidx, s->rd.nread_idx.p, s->rd.n_nreads * 4, hipMemcpyDeviceToHost));
    if (out_nascii && s->rd.n_nreads) HIP_TRY(c, hipMemcpy(out_nascii, s->rd.nread_ascii.p, s->rd.n_nreads * s->prm.read_len, hipMemcpyDeviceToHost));
    if (out_text && s->txt.have_pg) HIP_TRY(c, hipMemcpy(out_text, s->txt.pg2[0].p, s->txt.pg_words * 4, hipMemcpyDeviceToHost));
    return PGRC_OK;
}

// ---------------------------------------------------------------------------------------------------- the stage handle
extern "C" uint64_t pgrc_selftest_stage_bytes(void) { return DEC_STAGE_BYTES; }

// `bytes` bytes of `in` up with dec_upload_host and down again with dec_download_host into `out`, on a stage that the entry
// opens and closes (stagectx.h).  pinned_up / pinned_down: that side's host memory is page-locked -- allocated here and copied
// from `in` / into `out` -- so that the copy goes without the staging buffers; otherwise the caller's pageable array is used as
// it is.  The device buffer has a guard zone; *guards bit 0: it is intact.
extern "C" int pgrc_selftest_stage_roundtrip(pgrc_selftest *h, const void *in, uint64_t bytes, int pinned_up, int pinned_down, void *out, uint32_t *guards) {
    PgrcDev *c = &h->dev;
    *guards = 0;
    PgrcDeviceScope scope(c->device);
    if (!scope.ok) {
        c->err = "selftest: hipSetDevice failed";
        return PGRC_E_NO_DEVICE;
    }
    void *pin[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; k++)
        if ((k ? pinned_down : pinned_up) && hipHostMalloc(&pin[k], bytes + 16) != hipSuccess) {
            (void)hipGetLastError();
            if (pin[0]) (void)hipHostFree(pin[0]);
            c->err = "selftest: hipHostMalloc failed";
            return PGRC_E_ALLOC;
        }
    if (pin[0]) memcpy(pin[0], in, bytes);
    StBuf dbuf;
    PgrcStage s;
    std::string why;
    int e = pgrc_stage_open(&s, c->device, &why);
    if (e) {
        c->err = "selftest: " + why;
    } else {
        bool ok = false;
        hipError_t he = dbuf.alloc(bytes, ST_GUARD);
        if (he == hipSuccess) {
            if (!(e = dec_upload_host(&s, dbuf.p, pin[0] ? pin[0] : in, bytes))) e = dec_download_host(&s, pin[1] ? pin[1] : out, dbuf.p, bytes);
            if (!e) he = dbuf.intact(&ok);
        }
        if (he != hipSuccess) {
            s.err = hipGetErrorString(he);
            e = pgrc_hip_code(he);
        }
        if (e) c->err = "selftest: " + s.err;
        *guards = ok ? 1u : 0u;
        pgrc_stage_close(&s);
    }
    if (!e && pin[1]) memcpy(out, pin[1], bytes);
    for (void *p : pin)
        if (p) (void)hipHostFree(p);
    return e;
}

// ---------------------------------------------------------------------------------------------------- the verifier (verify.hip)
// Phases 2-4 of the MULTISET kind -- the union sort, the run structure, the byte compare of the pairs -- on keys and items of
// the caller: n_s source and n_d decoded items of item_bytes bytes each, one key per item.  counts: matched pairs, undecided
// pairs, unmatched source items, unmatched decoded items, the smallest unmatched source and decoded index (UINT64_MAX: none).
extern "C" int pgrc_selftest_verify_match(pgrc_selftest *h, const uint64_t *keys_s, const uint8_t *items_s, uint64_t n_s, const uint64_t *keys_d,
                                          const uint8_t *items_d, uint64_t n_d, uint32_t item_bytes, uint64_t counts[6]) {
    PgrcDev *c = &h->dev;
    if (!item_bytes) {
        c->err = "selftest: item_bytes is 0";
        return PGRC_E_PARAM;
    }
    pgrc_verify *v = nullptr;
    int e = pgrc_vf_open(c->device, item_bytes, &v);
    if (e) {
        c->err = std::string("selftest: ") + pgrc_verify_last_error(nullptr);
        return e;
    }
    PgrcDeviceScope scope(c->device);
    StBuf its, itd;
    hipError_t he = its.alloc(n_s * item_bytes, VF_PAD);
    if (he == hipSuccess) he = itd.alloc(n_d * item_bytes, VF_PAD);
    if (he == hipSuccess && n_s) he = hipMemcpy(its.p, items_s, n_s * item_bytes, hipMemcpyHostToDevice);
    if (he == hipSuccess && n_d) he = hipMemcpy(itd.p, items_d, n_d * item_bytes, hipMemcpyHostToDevice);
    if (he == hipSuccess && !(e = pgrc_vf_key_buffers(v, n_s + n_d))) {
        if (n_s) he = hipMemcpy(v->key[0].p, keys_s, n_s * 8, hipMemcpyHostToDevice);
        if (he == hipSuccess && n_d) he = hipMemcpy((uint64_t *)v->key[0].p + n_s, keys_d, n_d * 8, hipMemcpyHostToDevice);
    }
    if (he == hipSuccess && !e) {
        VfSide s{{its.p, nullptr}, {item_bytes, 0}, n_s}, d{{itd.p, nullptr}, {item_bytes, 0}, n_d};
        VfCounts r;
        if (!(e = pgrc_vf_match_keys(v, s, d, &r))) {
            const uint64_t out[6] = {r.matched, r.undecided, r.s_unmatched, r.d_unmatched, r.first_s, r.first_d};
            memcpy(counts, out, sizeof out);
        }
    }
    if (he != hipSuccess) {
        v->err = hipGetErrorString(he);
        e = pgrc_hip_code(he);
    }
    if (e) c->err = "selftest: " + v->err;
    pgrc_verify_end(v);
    return e;
}

// the next pgrc_verify_begin of the process (of THIS library: tests call its pgrc_verify_* entries) cuts its keys to `bits` bits
extern "C" void pgrc_selftest_verify_mask_next_begin(uint32_t bits) { pgrc_vf_mask_next_begin(bits); }
