// mempack.hip -- a text that is ALREADY in HBM as ASCII (an assembled pseudogenome, pgrc_asm_text_device) packed for the
// Pg-vs-Pg matcher (mem.hip) in one launch: the 2-bit words, the 16-bit-per-word N map and the flag word of k_mem_pack, forward
// or reverse-complemented (what SimplePgMatcher does on the host before matchTexts, matching/SimplePgMatcher.cpp:31-41, with
// the reference's complement table: N stays N).  DESIGN.md 4.21.
//
// The text may start at any byte address.  A block takes MP_TILE_WORDS output words = MP_TILE_WORDS * 16 input bytes at a
// time: the 16-byte-aligned pieces of HBM that cover them go to an LDS tile with one 16-byte load a lane (a wave reads 1 KiB
// of consecutive bytes; k_mem_pack's lanes read single bytes 16 apart), the first and the last piece of the text byte by byte,
// since they may reach outside it; then every lane builds one word from two aligned 16-byte LDS reads, shifted by the
// text's misalignment, which is the same for every tile.  In the reversed form output symbol i is the complement of input byte
// n - 1 - i: the tile is the same, the lanes walk it from its end.
//
// A single pass bound by HBM: 1 byte read, 3/8 byte written a symbol.
#include "ctx.h"
#include "devutil.h"

#define MP_TPB 256
#define MP_TILE_WORDS MP_TPB                 // one output word a lane
#define MP_TILE_BYTES (MP_TILE_WORDS * 16)

__device__ __forceinline__ uint32_t mp_spread16(uint32_t x) {                       // bit i -> bit 2i
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

// dwords D .. D + 4 of q[8], shifted right by `sh` bits into four dwords (D a constant: no indexed registers)
template <int D>
__device__ __forceinline__ void mp_take(const uint32_t (&q)[8], uint32_t sh, uint32_t (&r)[4]) {
#pragma unroll
    for (int k = 0; k < 4; k++) r[k] = funnel_r(q[D + k], q[D + k + 1], sh);
}

// words[0 .. words_out): the packed text in its first (n + 15) / 16 words, zero behind it (the pad that the matcher's windows
// read).  nmap: as many 16-bit masks of the N's, or null.  flags: bit 0 a symbol outside ACGNT, bit 1 an N.
template <bool REV>
__global__ void __launch_bounds__(MP_TPB)
k_mem_pack_dev(const uint8_t *__restrict__ ascii, uint64_t n, uint32_t *__restrict__ words, uint16_t *__restrict__ nmap, uint64_t words_out,
               uint32_t *flags) {
    __shared__ uint4 tile[MP_TILE_WORDS + 1];                                      // 16-byte pieces; one more for the misalignment
    const uint64_t ntiles = (words_out + MP_TILE_WORDS - 1) / MP_TILE_WORDS;
    // Forward, tile T holds the bytes [16 * W0, 16 * W0 + MP_TILE_BYTES) of the text, W0 = T * MP_TILE_WORDS; reversed, the
    // bytes [n - 16 * W0 - MP_TILE_BYTES, n - 16 * W0), which may begin before the text.  Either start is a multiple of 16
    // away from the text's first byte (forward) or from the byte behind its last (reversed): one misalignment for all tiles.
    const uint32_t mis = (uint32_t)(((uintptr_t)ascii + (REV ? n : 0ull)) & 15u);
    const uint32_t sh = (mis & 3u) * 8u;
    uint32_t fl = 0;
    for (uint64_t T = blockIdx.x; T < ntiles; T += gridDim.x) {
        const uint64_t W0 = T * MP_TILE_WORDS;
        const int64_t s0 = REV ? (int64_t)n - (int64_t)(16 * W0) - MP_TILE_BYTES : (int64_t)(16 * W0);   // text position of the tile's first byte
        const int64_t p0 = s0 - (int64_t)mis;                                     // ... of LDS piece 0: an aligned address
        for (uint32_t j = threadIdx.x; j < MP_TILE_WORDS + 1; j += MP_TPB) {
            const int64_t lo = p0 + 16 * (int64_t)j;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (lo >= 0 && lo + 16 <= (int64_t)n) {
                v = *reinterpret_cast<const uint4 *>(ascii + lo);
            } else if (lo + 16 > 0 && lo < (int64_t)n) {                         // the text's head or tail: only the bytes inside it
                uint32_t b[4] = {0, 0, 0, 0};
                for (int k = 0; k < 16; k++)
                    if (lo + k >= 0 && lo + k < (int64_t)n) b[k >> 2] |= (uint32_t)ascii[lo + k] << (8 * (k & 3));
                v = make_uint4(b[0], b[1], b[2], b[3]);
            }
            tile[j] = v;
        }
        __syncthreads();
        const uint64_t w = W0 + threadIdx.x;
        if (w < words_out) {
            const uint32_t cnt = 16 * w >= n ? 0u : (uint32_t)min((uint64_t)16, n - 16 * w);   // symbols of this word
            // its 16 bytes, in text order: at byte mis + 16 * x of the tile, x = the lane (forward) or counted from the end
            const uint32_t x = REV ? MP_TILE_WORDS - 1 - threadIdx.x : threadIdx.x;
            const uint4 a = tile[x], b = tile[x + 1];
            const uint32_t q[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t r[4];
            switch (mis >> 2) {                                                   // (uniform)
            case 0: mp_take<0>(q, sh, r); break;
            case 1: mp_take<1>(q, sh, r); break;
            case 2: mp_take<2>(q, sh, r); break;
            default: mp_take<3>(q, sh, r); break;
            }
            // byte k is symbol k of the word (forward) or symbol 15 - k (reversed): the bytes that count
            const uint32_t valid = cnt == 0 ? 0u : REV ? (0xFFFFu << (16 - cnt)) & 0xFFFFu : 0xFFFFu >> (16 - cnt);
            uint32_t out = 0, nb = 0, bad = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const uint32_t c = (r[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                uint32_t code = (c >> 1) & 3u;
                code ^= code >> 1;                                                // A0 C1 G2 T3
                const bool is_n = c == 'N';
                if (is_n) { nb |= 1u << k; code = 0; }
                else if (c != 'A' && c != 'C' && c != 'G' && c != 'T') bad |= 1u << k;
                out |= code << (2 * k);
            }
            nb &= valid;
            if (REV) {
                nb = __brev(nb) >> 16;
                out = revcomp_word(out) & ~(3u * mp_spread16(nb));                // an N packs as code 0 on either strand
            }
            out &= cnt == 16 ? 0xFFFFFFFFu : (1u << (2 * cnt)) - 1u;
            words[w] = out;
            if (nmap) nmap[w] = (uint16_t)nb;
            if (bad & valid) fl |= 1u;
            if (nb) fl |= 2u;
        }
        __syncthreads();                                                          // (the next tile overwrites the LDS)
    }
    if (fl) atomicOr(flags, fl);
}

int pgrc_launch_mem_pack_device(PgrcDev *c, const uint8_t *d_ascii, uint64_t n, bool reversed, uint32_t *d_words, uint16_t *d_nmap, uint64_t words_out,
                                uint32_t *d_flags, uint32_t block_cap) {
    if (!words_out) return PGRC_OK;
    const uint64_t ntiles = (words_out + MP_TILE_WORDS - 1) / MP_TILE_WORDS;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(ntiles, block_cap ? std::min(block_cap, 65536u) : 65536u);
    if (reversed) hipLaunchKernelGGL(k_mem_pack_dev<true>, dim3(grid), dim3(MP_TPB), 0, c->stream, d_ascii, n, d_words, d_nmap, words_out, d_flags);
    else hipLaunchKernelGGL(k_mem_pack_dev<false>, dim3(grid), dim3(MP_TPB), 0, c->stream, d_ascii, n, d_words, d_nmap, words_out, d_flags);
    HIP_TRY(c, hipGetLastError());
    return PGRC_OK;
}
