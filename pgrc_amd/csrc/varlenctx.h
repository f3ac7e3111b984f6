// varlenctx.h -- the coder behind include/pgrc_varlen.h (varlen.hip), as the two stages that feed it and read it see it:
// pgmap.hip (pgrc_mem_encode_mapped) and restore.hip (pgrc_decode_set_mapped_text_coded).
#pragma once

#include <string>

#include "ctx.h"
#include "pgrc_varlen.h"

// the tables of the encoder, copied to LDS by every block.  Indexes are the low three bits of up to four symbols, three bits
// a place, the first symbol lowest.  t4 .. t1: the four rungs of the reference's look-up (0 = not in the book); e: what the
// rungs give for a window with at least four bytes left, the code in the low byte and the step above it
struct VlTables {
    uint16_t e[4096];
    uint8_t t3[512];
    uint8_t t2[64];
    uint8_t t1[8];
    uint8_t sym[8];            // the book's symbol with these low three bits, 0 = none
};
static_assert(sizeof(VlTables) % 16 == 0, "copied to LDS as uint4");

// the decoder's: a code's symbols (little endian) and their number
struct VlBook {
    uint32_t bytes[256];
    uint8_t len[256];
};
static_assert(sizeof(VlBook) % 16 == 0, "copied to LDS as uint4");

struct pgrc_varlen : PgrcDev {
    PhaseEvents<4> ev;
    uint32_t ncodes = 0;
    VlTables tab{};
    uint8_t t4[4096]{};        // (host only: e is made from it)
    VlBook book{};
    DevBuf d_tab, d_book, d_src, d_coded, d_text, d_bmap, d_bent, d_bcnt, d_bsum, d_bbase, d_fold, d_flag;
    pgrc_varlen_times tm{};
};
