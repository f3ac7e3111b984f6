"""The hand-over (pack.hip, the host packer and append_rows of api.hip) against numpy: plain references of every format it
reads and writes, written from the formats (ctx.h, include/pgrc_match.h), and the ctypes binding of libpgrc_selftest.so's
hand-over entries on top of prim_util.lib().  tests/test_handover_reference.py holds the references to the oracle's packer,
and through it to the compiled reference, on the CPU.

One symbol-level core -- an (n, L) array of codes A0 C1 G2 T3 and an N mask of the same shape -- and every format derived from
it by arithmetic on the symbol index i:
    word-major array   word i // 16 of a read, bits 2 * (i % 16); an N packs as code 0
    ACGT bytes         byte i // 4, most significant pair first
    ACGNT bytes        byte i // 3, base-5 digits A0 C1 G2 N3 T4, most significant first, pad digit 0
    flag               0 no N; 3 one to four N's, their positions as the bytes of a word, lowest first, 0xFF for none; 1 five
                       or more N's (no position word)
    side list          the flagged reads' indexes, ascending, and their ASCII rows in that order"""
import ctypes as C

import numpy as np

import prim_util as pu

_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
_CODE[ord("N")] = 4
ASCII = np.frombuffer(b"ACGT", dtype=np.uint8)
N = ord("N")


# ---------------------------------------------------------------------------------------------- reads
def symbols(rows):
    """ASCII rows (n, L) over ACGNT -> (codes 0..3 with 0 at an N, N mask)"""
    rows = np.asarray(rows, dtype=np.uint8)
    c = _CODE[rows]
    assert (c <= 4).all(), "a symbol outside ACGNT"
    nmask = c == 4
    return np.where(nmask, 0, c).astype(np.uint8), nmask


def ascii_rows(codes, nmask):
    return np.where(nmask, np.uint8(N), ASCII[codes]).astype(np.uint8)


def read_words(codes):
    """(nw, n) u32: word w of read r at [w, r]"""
    n, L = codes.shape
    out = np.zeros(((L + 15) // 16, n), dtype=np.uint32)
    for i in range(L):
        out[i // 16] |= codes[:, i].astype(np.uint32) << np.uint32(2 * (i % 16))
    return out


def acgt_bytes(codes):
    n, L = codes.shape
    out = np.zeros((n, (L + 3) // 4), dtype=np.uint8)
    for i in range(L):
        out[:, i // 4] |= codes[:, i] << np.uint8(2 * (3 - i % 4))
    return out


def acgnt_bytes(codes, nmask):
    n, L = codes.shape
    digit = np.where(nmask, 3, np.where(codes == 3, 4, codes)).astype(np.uint8)
    out = np.zeros((n, (L + 2) // 3), dtype=np.uint8)
    for i in range(L):
        out[:, i // 3] += digit[:, i] * np.uint8(5 ** (2 - i % 3))
    return out


def flags_npos(nmask):
    """-> (flag u8[n], npos u32[n]); npos means something where flag == 3 only"""
    n, L = nmask.shape
    cnt = nmask.sum(axis=1)
    flag = np.where(cnt == 0, 0, np.where(cnt <= 4, 3, 1)).astype(np.uint8)
    at = np.sort(np.where(nmask, np.arange(L)[None, :], 255), axis=1)[:, :4].astype(np.uint32)
    at = np.concatenate([at, np.full((n, 4 - at.shape[1]), 255, dtype=np.uint32)], axis=1)
    npos = at[:, 0] | at[:, 1] << np.uint32(8) | at[:, 2] << np.uint32(16) | at[:, 3] << np.uint32(24)
    return flag, npos.astype(np.uint32)


def side_list(rows, flag):
    idx = np.flatnonzero(flag).astype(np.uint32)
    return idx, np.ascontiguousarray(np.asarray(rows, dtype=np.uint8)[idx])


def unpack_reads(words, flag, npos, L):
    """the ASCII rows that a word-major array (nw, n), the flags and the position words describe; a read flagged 1 comes back
    with 'A' where its N's were (its positions are not kept)"""
    n = words.shape[1]
    codes = np.zeros((n, L), dtype=np.uint8)
    for i in range(L):
        codes[:, i] = (words[i // 16] >> np.uint32(2 * (i % 16))) & np.uint32(3)
    nmask = np.zeros((n, L), dtype=bool)
    for k in range(4):
        b = (npos >> np.uint32(8 * k)) & np.uint32(0xFF)
        r = np.flatnonzero((flag == 3) & (b != 0xFF))
        nmask[r, b[r]] = True
    return ascii_rows(codes, nmask)


def rows_of(rows, kind):
    """the host rows of one hand-over format: kind 0 ASCII, 4 the ACGT packing, 5 the ACGNT packing"""
    if kind == 0:
        return np.ascontiguousarray(rows, dtype=np.uint8)
    codes, nmask = symbols(rows)
    if kind == 4:
        assert not nmask.any()
        return acgt_bytes(codes)
    return acgnt_bytes(codes, nmask)


def read_state(rows):
    """what a context holds of the ASCII rows (n, L) after the hand-over, in any of the three formats"""
    codes, nmask = symbols(rows)
    flag, npos = flags_npos(nmask)
    idx, nascii = side_list(rows, flag)
    return {"words": read_words(codes), "flag": flag, "npos": npos, "nidx": idx, "nascii": nascii, "n_many": int((flag == 1).sum())}


# ---------------------------------------------------------------------------------------------- text
def text_codes(ascii_1d):
    c = _CODE[np.asarray(ascii_1d, dtype=np.uint8)]
    assert (c < 4).all(), "a symbol outside ACGT"
    return c


def pack_codes(codes):
    """symbol i at bits 2 * (i % 16) of word i // 16, on bytes: four symbols to a byte, lowest first, four bytes to a word"""
    c = np.concatenate([codes, np.zeros((-codes.size) % 16, dtype=np.uint8)]).reshape(-1, 4)
    b = c[:, 0] | c[:, 1] << np.uint8(2) | c[:, 2] << np.uint8(4) | c[:, 3] << np.uint8(6)
    return np.ascontiguousarray(b).view("<u4")


def pack_text(ascii_1d):
    return pack_codes(text_codes(ascii_1d))


def revcomp_text(ascii_1d):
    """the packed reverse complement: symbol i is 3 - symbol G - 1 - i"""
    return pack_codes(np.uint8(3) - text_codes(ascii_1d)[::-1])


def random_text(G, seed):
    return ASCII[np.random.default_rng(seed).integers(0, 4, G, dtype=np.uint8)]


# ---------------------------------------------------------------------------------------------- the library
_bound = False


def lib():
    global _bound
    L = pu.lib()
    if not _bound:
        vp, u32, u64, i32, pu32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(C.c_uint32)
        L.pgrc_selftest_pack_text.argtypes = [vp, vp, u64, vp, pu32, pu32]
        L.pgrc_selftest_revcomp.argtypes = [vp, vp, u64, vp, pu32]
        L.pgrc_selftest_pack_reads.argtypes = [vp, i32, vp, u64, u64, u32, u64, u64, vp, vp, vp, pu32, pu32]
        L.pgrc_selftest_nrows_ascii.argtypes = [vp, vp, u64, vp, u64, u32, vp, pu32]
        L.pgrc_selftest_reads_state.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp]
        _bound = True
    return L


_ptr = pu._ptr


class HandOver(pu.SelfTest):
    """the hand-over entries of libpgrc_selftest.so on one device"""

    def __init__(self, device=0):
        lib()
        super().__init__(device)

    def pack_text(self, ascii_1d):
        """-> (words, error flag, guards); guards == 3: intact"""
        a = np.ascontiguousarray(ascii_1d, dtype=np.uint8)
        out = np.zeros((a.size + 15) // 16, dtype=np.uint32)
        err, g = C.c_uint32(7), C.c_uint32(0)
        self._check(lib().pgrc_selftest_pack_text(self.h, _ptr(a), a.size, _ptr(out), C.byref(err), C.byref(g)), "pack_text")
        return out, err.value, g.value

    def revcomp(self, words, G):
        """-> (words of the reverse complement, guards); guards == 1: intact"""
        w = np.ascontiguousarray(words, dtype=np.uint32)
        assert w.size == (G + 15) // 16
        out = np.zeros(w.size, dtype=np.uint32)
        g = C.c_uint32(0)
        self._check(lib().pgrc_selftest_revcomp(self.h, _ptr(w), G, _ptr(out), C.byref(g)), "revcomp")
        return out, g.value

    def pack_reads(self, kind, rows, first, L, n_total, stride):
        """-> (words (nw, stride), nflag[n_total], npos[n_total], error flag, guards); guards == 15: intact"""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        nw = (L + 15) // 16
        words = np.zeros((nw, stride), dtype=np.uint32)
        nflag, npos = np.zeros(n_total, dtype=np.uint8), np.zeros(n_total, dtype=np.uint32)
        err, g = C.c_uint32(7), C.c_uint32(0)
        self._check(lib().pgrc_selftest_pack_reads(self.h, kind, _ptr(rows), first, rows.shape[0], L, n_total, stride, _ptr(words), _ptr(nflag), _ptr(npos),
                                                   C.byref(err), C.byref(g)), "pack_reads")
        return words, nflag, npos, err.value, g.value

    def nrows_ascii(self, packed, local_idx, L):
        """-> (ASCII rows (count, L), guards); guards == 1: intact"""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        idx = np.ascontiguousarray(local_idx, dtype=np.uint32)
        out = np.zeros((idx.size, L), dtype=np.uint8)
        g = C.c_uint32(0)
        self._check(lib().pgrc_selftest_nrows_ascii(self.h, _ptr(packed), packed.shape[0], _ptr(idx), idx.size, L, _ptr(out), C.byref(g)), "nrows_ascii")
        return out, g.value

    def reads_state(self, ctx, multi=False, text=False):
        """what the product's MatchContext holds (multi: it was made with `devices`): one dict per shard (one for a single-device context) with n, stride, nw,
        n_nreads, n_many, lo, hi, words (nw, stride), flag, npos (None where it was never allocated), nidx, nascii, and the
        shard's forward text where `text`"""
        out = []
        for r in range(len(ctx.shards()) if multi else 1):
            shard = r if multi else -1
            info = np.zeros(10, dtype=np.uint64)
            self._check(lib().pgrc_selftest_reads_state(self.h, ctx._h, shard, _ptr(info), None, None, None, None, None, None), "reads_state")
            n, stride, nw, n_nreads, n_many, has_npos, pg_words, lo, hi, _ = (int(x) for x in info)
            d = {"n": n, "stride": stride, "nw": nw, "n_nreads": n_nreads, "n_many": n_many, "lo": lo, "hi": hi,
                 "words": np.zeros((nw, stride), dtype=np.uint32), "flag": np.zeros(n, dtype=np.uint8),
                 "npos": np.zeros(n, dtype=np.uint32) if has_npos else None, "nidx": np.zeros(n_nreads, dtype=np.uint32),
                 "nascii": np.zeros((n_nreads, ctx.read_len), dtype=np.uint8), "text": np.zeros(pg_words, dtype=np.uint32) if text else None}
            self._check(lib().pgrc_selftest_reads_state(self.h, ctx._h, shard, _ptr(info), _ptr(d["words"]), _ptr(d["flag"]),
                                                        _ptr(d["npos"]) if has_npos else None, _ptr(d["nidx"]), _ptr(d["nascii"]),
                                                        _ptr(d["text"]) if text else None), "reads_state")
            out.append(d)
        return out
