// scanops.h -- every prefix scan of the library: one scan over the threads of a block, and one device-wide scan in three kernels
// built on it (per-block folds, one block that scans the folds, per-block rescan with the carried-in prefix).  Any associative
// operator over u32, u64 or a small struct; the operator need not commute (the folds keep the input order).  No library scan
// (DESIGN.md 4.10).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#define SCO_TPB 256
#define SCO_EPT 16
#define SCO_EPB (SCO_TPB * SCO_EPT)

struct ScoIdentity {
    template <typename T>
    __device__ T operator()(T x) const { return x; }
};
struct ScoPlus {
    template <typename T>
    __device__ T operator()(T a, T b) const { return a + b; }
};

// A weak order of five items in a u32: the dense rank of item g (0 .. 4) in bits [3g, 3g + 3).  sco_dense5 ranks five keys
// (the number of distinct smaller keys).  ScoWeakOrder5 is "a, then b": the items sorted by b's ranks, ties kept in a's order
// -- the dense ranks of the pairs (b[g], a[g]).  Associative, not commutative; the all-equal order 0 is its identity (pgovl.hip:
// the order of the groups in front of every run of equal suffixes).
__host__ __device__ __forceinline__ uint32_t sco_dense5(const uint32_t (&key)[5]) {
    uint32_t w = 0;
#pragma unroll
    for (int g = 0; g < 5; g++) {
        uint32_t rank = 0;
#pragma unroll
        for (int h = 0; h < 5; h++) {
            bool first = key[h] < key[g];
#pragma unroll
            for (int h2 = 0; h2 < h; h2++) first = first && key[h2] != key[h];
            rank += first ? 1u : 0u;
        }
        w |= rank << (3 * g);
    }
    return w;
}
struct ScoWeakOrder5 {
    __host__ __device__ uint32_t operator()(uint32_t a, uint32_t b) const {
        uint32_t key[5];
#pragma unroll
        for (int g = 0; g < 5; g++) key[g] = (((b >> (3 * g)) & 7u) << 3) | ((a >> (3 * g)) & 7u);
        return sco_dense5(key);
    }
};
#define SCO_WEAK5_SYMBOL_ORDER (0u | 1u << 3 | 2u << 6 | 3u << 9 | 4u << 12)

// The same fold over segments: an element with SCO_WEAK5_RESET set forgets everything in front of it (its order already holds
// whatever a segment starts from), and the bit stays on the fold of anything that holds such an element.  Associative; 0 is
// still the identity (pgovl.hip under the parallel rule: the order of the groups starts anew with every block).
#define SCO_WEAK5_RESET 0x80000000u
struct ScoWeakOrder5Reset {
    __host__ __device__ uint32_t operator()(uint32_t a, uint32_t b) const {
        if (b & SCO_WEAK5_RESET) return b;
        return (a & SCO_WEAK5_RESET) | ScoWeakOrder5{}(a & ~SCO_WEAK5_RESET, b & ~SCO_WEAK5_RESET);
    }
};

// A map {0..3} -> {0..3} in 8 bits of a u32: the image of e in bits [2e, 2e + 2).  ScoMap4 is "a, then b": e -> b[a[e]].
// Associative, not commutative; SCO_MAP4_IDENTITY is its identity (varlen.hip: a tile of the text takes the offset at which
// the parse enters it to the offset at which the parse leaves it).
struct ScoMap4 {
    __host__ __device__ uint32_t operator()(uint32_t a, uint32_t b) const {
        uint32_t r = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) r |= ((b >> (2 * ((a >> (2 * e)) & 3u))) & 3u) << (2 * e);
        return r;
    }
};
#define SCO_MAP4_IDENTITY 0xE4u

// a value of any size that is a multiple of 4 bytes, from the lane `o` below, word by word
template <typename T>
__device__ __forceinline__ T sco_shfl_up(T v, int o) {
    static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "shuffled as 32-bit words");
    uint32_t w[sizeof(T) / 4];
    memcpy(w, &v, sizeof(T));
#pragma unroll
    for (uint32_t k = 0; k < sizeof(T) / 4; k++) w[k] = __shfl_up(w[k], o, 64);
    memcpy(&v, w, sizeof(T));
    return v;
}

// The block's values in thread order: returns the fold of everything BEFORE this thread (ident for thread 0), *total = the fold
// of the whole block.  NWV = waves of the block (0: blockDim.x >> 6); smem: one T per wave.  SYNC_AFTER = false leaves out the
// barrier that lets smem be written again: for a caller that has a barrier of its own before it next touches smem.
// With ScoPlus the exclusive value is the inclusive one minus the thread's own, which saves the shuffle of the general form.
template <int NWV = 0, bool SYNC_AFTER = true, typename T, typename Op>
__device__ __forceinline__ T sco_block_exclusive(T v, Op op, T ident, T *smem, T *total) {
    constexpr bool SUM = std::is_same<Op, ScoPlus>::value;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = NWV ? (uint32_t)NWV : blockDim.x >> 6;
    T inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const T u = sco_shfl_up(inc, o);
        if (lane >= (uint32_t)o) inc = op(u, inc);
    }
    if (lane == 63) smem[wv] = inc;
    __syncthreads();
    T woff = ident, tot = ident;
    for (uint32_t k = 0; k < nwv; k++) {
        const T s = smem[k];
        if (k < wv) woff = op(woff, s);
        tot = op(tot, s);
    }
    if (SYNC_AFTER) __syncthreads();
    *total = tot;
    if constexpr (SUM) {
        return woff + inc - v;
    } else {
        T before = sco_shfl_up(inc, 1);
        if (lane == 0) before = ident;
        return op(woff, before);
    }
}

// the sum over u32 or u64
template <int NWV = 0, bool SYNC_AFTER = true, typename T>
__device__ __forceinline__ T sco_block_sum(T v, T *smem, T *total) {
    return sco_block_exclusive<NWV, SYNC_AFTER>(v, ScoPlus{}, (T)0, smem, total);
}

// ---------------------------------------------------------------- the device-wide scan
template <typename T, typename In, typename Xf>
struct ScoLoad {            // xf(in[i]), widened to T
    const In *p;
    Xf xf;
    __device__ T operator()(uint64_t i) const { return (T)xf(p[i]); }
};
template <typename T>
struct ScoStore {
    T *p;
    __device__ void operator()(uint64_t i, T v) const { p[i] = v; }
};

// a thread's SCO_EPT consecutive elements from `base` on (ident past the end), all loads first; plain u32 input in whole
// blocks is read as four uint4
template <typename T, typename In>
__device__ __forceinline__ void sco_load_thread(const In &in, uint64_t base, uint64_t n, T ident, T (&v)[SCO_EPT]) {
#pragma unroll
    for (int k = 0; k < SCO_EPT; k++) v[k] = (base + k < n) ? in(base + k) : ident;
}
__device__ __forceinline__ void sco_load_thread(const ScoLoad<uint32_t, uint32_t, ScoIdentity> &in, uint64_t base, uint64_t n, uint32_t ident,
                                                uint32_t (&v)[SCO_EPT]) {
    if (base + SCO_EPT <= n) {
        const uint4 *p = reinterpret_cast<const uint4 *>(in.p + base);
#pragma unroll
        for (int k = 0; k < SCO_EPT / 4; k++) {
            const uint4 q = p[k];
            v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < SCO_EPT; k++) v[k] = (base + k < n) ? in.p[base + k] : ident;
    }
}

// in: index -> T; out: (index, T); SCO_TPB threads x SCO_EPT consecutive elements.  fold[b] = the fold of block b
template <typename T, typename In, typename Op>
__global__ void __launch_bounds__(SCO_TPB) k_sco_folds(In in, uint64_t n, Op op, T ident, T *__restrict__ fold) {
    __shared__ T smem[SCO_TPB / 64];
    const uint64_t base = (uint64_t)blockIdx.x * SCO_EPB + (uint64_t)threadIdx.x * SCO_EPT;
    T v[SCO_EPT], s = ident;
    sco_load_thread(in, base, n, ident, v);
#pragma unroll
    for (int k = 0; k < SCO_EPT; k++) s = op(s, v[k]);
    T tot;
    sco_block_exclusive<SCO_TPB / 64>(s, op, ident, smem, &tot);
    if (threadIdx.x == 0) fold[blockIdx.x] = tot;
}

// one block: fold[i] = start, then the blocks before i; fold[nb] = start, then everything
template <typename T, typename Op>
__global__ void __launch_bounds__(SCO_TPB) k_sco_carry(T *fold, uint64_t nb, Op op, T ident, T start) {
    __shared__ T smem[SCO_TPB / 64];
    T run = start;
    for (uint64_t b0 = 0; b0 < nb; b0 += SCO_TPB) {
        const uint64_t i = b0 + threadIdx.x;
        const T v = i < nb ? fold[i] : ident;
        T tot;
        const T ex = sco_block_exclusive<SCO_TPB / 64>(v, op, ident, smem, &tot);
        if (i < nb) fold[i] = op(run, ex);
        run = op(run, tot);
    }
    if (threadIdx.x == 0) fold[nb] = run;
}

template <bool INCLUSIVE, bool TOTAL_AT_N, typename T, typename In, typename Op, typename Out>
__global__ void __launch_bounds__(SCO_TPB) k_sco_write(In in, uint64_t n, Op op, T ident, const T *__restrict__ fold, Out out) {
    __shared__ T smem[SCO_TPB / 64];
    const uint64_t base = (uint64_t)blockIdx.x * SCO_EPB + (uint64_t)threadIdx.x * SCO_EPT;
    T v[SCO_EPT], s = ident;
#pragma unroll
    for (int k = 0; k < SCO_EPT; k++) {
        v[k] = (base + k < n) ? in(base + k) : ident;
        s = op(s, v[k]);
    }
    T tot;
    T acc = op(fold[blockIdx.x], sco_block_exclusive<SCO_TPB / 64>(s, op, ident, smem, &tot));
#pragma unroll
    for (int k = 0; k < SCO_EPT; k++) {
        const T inc = op(acc, v[k]);
        if (base + k < n) out(base + k, INCLUSIVE ? inc : acc);
        acc = inc;
    }
    if (TOTAL_AT_N && blockIdx.x == 0 && threadIdx.x == 0) out(n, fold[gridDim.x]);
}

template <typename T, typename Out>
__global__ void k_sco_empty(Out out, T start) { out(0, start); }

// elements of T the scan of n values needs as scratch
static inline uint64_t sco_scratch_elems(uint64_t n) { return (n + SCO_EPB - 1) / SCO_EPB + 1; }

// out(i, fold of start, in(0), ..., in(i)) (INCLUSIVE) or out(i, fold of start, in(0), ..., in(i-1)) for every i < n; the
// exclusive form with TOTAL_AT_N also gives out(n, fold of start and everything).  A block calls in() for all its elements
// before it calls out(), so out may overwrite what in reads at the same index.  d_fold: sco_scratch_elems(n) elements.  On
// `stream`, no synchronisation.
template <bool INCLUSIVE, bool TOTAL_AT_N, typename T, typename In, typename Op, typename Out>
static inline hipError_t sco_device_scan(hipStream_t stream, In in, uint64_t n, Op op, T ident, T start, Out out, T *d_fold) {
    constexpr bool TOTAL = TOTAL_AT_N && !INCLUSIVE;
    if (!n) {
        if (TOTAL) hipLaunchKernelGGL((k_sco_empty<T, Out>), dim3(1), dim3(1), 0, stream, out, start);
        return hipGetLastError();
    }
    const uint64_t nb = (n + SCO_EPB - 1) / SCO_EPB;
    hipLaunchKernelGGL((k_sco_folds<T, In, Op>), dim3((uint32_t)nb), dim3(SCO_TPB), 0, stream, in, n, op, ident, d_fold);
    hipLaunchKernelGGL((k_sco_carry<T, Op>), dim3(1), dim3(SCO_TPB), 0, stream, d_fold, nb, op, ident, start);
    hipLaunchKernelGGL((k_sco_write<INCLUSIVE, TOTAL, T, In, Op, Out>), dim3((uint32_t)nb), dim3(SCO_TPB), 0, stream, in, n, op, ident, (const T *)d_fold, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------- the forms over arrays
// out[i] = fold of xf(in[0 .. i]) (INCLUSIVE) or of xf(in[0 .. i-1]) with ident in front, in u32; in and out may be the same array
template <bool INCLUSIVE, typename In, typename Xf, typename Op>
static inline hipError_t sco_scan(hipStream_t stream, const In *in, uint32_t *out, uint64_t n, Xf xf, Op op, uint32_t ident, uint32_t *d_fold) {
    return sco_device_scan<INCLUSIVE, false>(stream, ScoLoad<uint32_t, In, Xf>{in, xf}, n, op, ident, ident, ScoStore<uint32_t>{out}, d_fold);
}

// sums of u8 / u16 / u32 / u64 values in u64; the exclusive form also writes out[n] = the total
template <bool INCLUSIVE, typename In>
static inline hipError_t sco_sum_u64(hipStream_t stream, const In *in, uint64_t n, uint64_t *out, uint64_t *d_fold) {
    return sco_device_scan<INCLUSIVE, true>(stream, ScoLoad<uint64_t, In, ScoIdentity>{in, ScoIdentity{}}, n, ScoPlus{}, (uint64_t)0, (uint64_t)0, ScoStore<uint64_t>{out}, d_fold);
}
