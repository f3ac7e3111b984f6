"""Pg-vs-Pg matching on texts that are already on the device (pgrc_mem_set_src_device, pgrc_mem_match_texts_device; DESIGN.md
4.21): the numpy reference of the packing kernel (mempack.hip) and the ctypes binding of its entry in libpgrc_selftest.so.

The reference is written from the layout, by arithmetic on the symbol index i, not from the kernel:
    symbol i       forward: byte i of the text; reversed: the complement (A<->T, C<->G, N stays N) of byte n - 1 - i
    word i // 16   its code A0 C1 G2 T3 at bits 2 * (i % 16); an N packs as code 0
    N map          bit i % 16 of the 16-bit mask i // 16: symbol i is an N
    flags          bit 0: some byte is outside ACGNT (the words and the map then mean nothing); bit 1: some byte is an N
    pad            zero bits above the last symbol, PAD_WORDS zero words (and masks) behind the last word
tests/test_memdev_reference.py holds it to oracle.revcomp_ascii and to the forward packers that exist already, on the CPU."""
import ctypes as C

import numpy as np

import prim_util as pu

PAD_WORDS = 32              # ctx.h PGRC_PG_PAD_WORDS
TILE_BYTES = 4096           # mempack.hip MP_TILE_BYTES: input bytes of one block's LDS tile
N = ord("N")
ASCII = np.frombuffer(b"ACGT", dtype=np.uint8)

_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
_CODE[N] = 4


def pack_ref(ascii_1d, reversed_, pad_words=PAD_WORDS):
    """-> (words u32[ceil(n / 16) + pad_words], nmap u16[the same], flags)"""
    a = np.ascontiguousarray(ascii_1d, dtype=np.uint8)
    n = a.size
    i = np.arange(n, dtype=np.int64)
    c = _CODE[a[n - 1 - i] if reversed_ else a]
    isn, bad = c == 4, c == 255
    if reversed_:
        c = np.uint8(3) - np.minimum(c, 3)
    c = np.where(isn | bad, 0, c).astype(np.uint32)
    nwords = (n + 15) // 16
    grid = np.zeros((nwords + pad_words) * 16, dtype=np.uint32)
    grid[:n] = c
    shifts = (2 * np.arange(16, dtype=np.uint32))[None, :]
    words = (grid.reshape(-1, 16) << shifts).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    ngrid = np.zeros((nwords + pad_words) * 16, dtype=np.uint32)
    ngrid[:n] = isn
    nmap = (ngrid.reshape(-1, 16) << np.arange(16, dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint16)
    return words, nmap, (1 if bad.any() else 0) | (2 if isn.any() else 0)


def random_text(n, seed, n_at=(), bad_at=None):
    """random ACGT with N at the positions n_at (those inside the text) and one byte outside ACGNT at bad_at"""
    t = ASCII[np.random.default_rng(seed).integers(0, 4, n, dtype=np.uint8)]
    for p in n_at:
        if 0 <= p < n:
            t[p] = N
    if bad_at is not None:
        t[bad_at] = ord("%")
    return t


# ---------------------------------------------------------------------------------------------- the library
_bound = False


def lib():
    global _bound
    L = pu.lib()
    if not _bound:
        vp, u32, u64, i32, pu32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(C.c_uint32)
        L.pgrc_selftest_mem_pack_device.argtypes = [vp, vp, u64, i32, u32, i32, vp, vp, pu32, pu32]
        _bound = True
    return L


class MemPack(pu.SelfTest):
    """the packing kernel's entry of libpgrc_selftest.so on one device"""

    def __init__(self, device=0):
        lib()
        super().__init__(device)

    def pack(self, dev_ptr, n, reversed_, block_cap=0, with_nmap=True):
        """the n ASCII bytes at the device address dev_ptr -> (words, nmap, flags, guards); guards == 7: intact.  Without an N
        map the masks come back as fill bytes."""
        total = (n + 15) // 16 + PAD_WORDS
        words, nmap = np.zeros(total, dtype=np.uint32), np.zeros(total, dtype=np.uint16)
        fl, g = C.c_uint32(0xFF), C.c_uint32(0)
        self._check(lib().pgrc_selftest_mem_pack_device(self.h, C.c_void_p(int(dev_ptr)), n, int(bool(reversed_)), block_cap, int(bool(with_nmap)),
                                                        pu._ptr(words), pu._ptr(nmap), C.byref(fl), C.byref(g)), "mem_pack_device")
        return words, nmap, fl.value, g.value
