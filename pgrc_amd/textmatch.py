"""Host-side mirror of the reference's TextMatcher seam (matching/TextMatchers.h:53-61) over include/pgrc_mem.h:
Pg-vs-Pg exact matching (SimplePgMatcher's CopMEMMatcher) on the MI355X.  No compute here."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import PgrcMatchError, lib

UINT32_MAX = 0xFFFFFFFF


def _ascii(a) -> np.ndarray:
    if isinstance(a, (bytes, bytearray, str)):
        a = np.frombuffer(a.encode() if isinstance(a, str) else bytes(a), dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8)


class CopMEMMatcher:
    """CopMEMMatcher(srcText, srcLength, targetMatchLength, minMatchLength) as a TextMatcher
    (matching/copmem/CopMEMMatcher.cpp:571-591, :604-622)."""

    def __init__(self, srcText, targetMatchLength: int, minMatchLength: int = UINT32_MAX, device: int = -1):
        """srcText None: a matcher without a source yet; setSrcDevice gives it one that is already on the device."""
        self._h = C.c_void_p()
        rc = lib.pgrc_mem_create(int(targetMatchLength), int(minMatchLength), int(device), C.byref(self._h))
        if rc:
            raise PgrcMatchError(rc, (lib.pgrc_mem_last_error(None) or b"").decode())
        self.targetMatchLength = int(targetMatchLength)
        self._src = None
        self._last_n2 = 0
        self._res_len = [0, 0, 0]            # the mapped texts kept on the device (markAndRemoveExactMatchesResident)
        if srcText is not None:
            self._src = _ascii(srcText)      # the library borrows the text: keep it alive
            self._ck(lib.pgrc_mem_set_src_ascii(self._h, self._src.ctypes.data_as(C.c_void_p), self._src.size))

    def _ck(self, rc: int) -> None:
        if rc:
            raise PgrcMatchError(rc, (lib.pgrc_mem_last_error(self._h) or b"").decode())

    def setSrcDevice(self, ptr: int, n: int) -> None:
        """the source text from `n` ASCII bytes at the raw device address `ptr` (PgAssembler.text_device()): packed into the
        matcher's own words and indexed; the buffer is not read after the call."""
        self._last_n2 = 0
        self._res_len = [0, 0, 0]
        self._ck(lib.pgrc_mem_set_src_device(self._h, C.c_void_p(int(ptr)), int(n)))
        self._src = None                     # (the host text of an earlier source is borrowed no longer)

    def _matches(self, out, cnt) -> np.ndarray:
        n = cnt.value
        res = np.zeros((n, 3), dtype=np.uint64)
        if n:
            res[:] = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(n * 3,)).reshape(n, 3)
            lib.pgrc_mem_free_matches(out)
        return res

    def matchTextsDevice(self, ptr: int, n2: int, destIsSrc: bool, revComplMatching: bool, minMatchLength: int | None = None) -> np.ndarray:
        """matchTexts over `n2` ASCII bytes at the raw device address `ptr`, the destination in its FORWARD orientation: with
        revComplMatching the library reverse-complements it on the device.  -> the matches that matchTexts returns for the
        host-reversed text.  With destIsSrc `ptr` may be 0."""
        self._last_n2 = 0
        out = C.POINTER(_lib.TextMatch)()
        cnt = C.c_uint64(0)
        self._ck(lib.pgrc_mem_match_texts_device(self._h, C.c_void_p(int(ptr)) if ptr else None, int(n2), int(bool(destIsSrc)),
                                                 int(bool(revComplMatching)),
                                                 self.targetMatchLength if minMatchLength is None else int(minMatchLength),
                                                 C.byref(out), C.byref(cnt)))
        self._last_n2 = int(n2)
        return self._matches(out, cnt)

    def matchTexts(self, destText, destIsSrc: bool, revComplMatching: bool, minMatchLength: int | None = None) -> np.ndarray:
        """-> uint64 array [count, 3] of (posSrcText, length, posDestText), discovery order.  destText is the text as
        SimplePgMatcher hands it over (already reverse-complemented when revComplMatching)."""
        d = _ascii(destText)
        self._last_n2 = 0
        out = C.POINTER(_lib.TextMatch)()
        cnt = C.c_uint64(0)
        self._ck(lib.pgrc_mem_match_texts(self._h, d.ctypes.data_as(C.c_void_p), d.size, int(bool(destIsSrc)),
                                          int(bool(revComplMatching)),
                                          self.targetMatchLength if minMatchLength is None else int(minMatchLength),
                                          C.byref(out), C.byref(cnt)))
        self._last_n2 = d.size               # (the destination stays on the device: markAndRemoveExactMatches maps it)
        return self._matches(out, cnt)

    def markAndRemoveExactMatches(self, matches, minMatchLength: int | None = None, mapped_out: np.ndarray | None = None):
        """markAndRemoveExactMatches (matching/SimplePgMatcher.cpp:69-148) of the destination of the last matchTexts call,
        which is still on the device: matches as matchTexts returns them (uint64 [count, 3]).
        -> (mapped, map_off, map_len, info) as uint8 arrays; info: marks, unique_matches, matched_symbols.  mapped_out: a uint8 buffer of at least the destination's length to write the mapped text into (it may
        be the destination text itself); the returned `mapped` is then a view of it."""
        mt = np.ascontiguousarray(np.asarray(matches, dtype=np.uint64).reshape(-1, 3))
        n2 = self._last_n2
        buf = np.empty(max(n2, 1), dtype=np.uint8) if mapped_out is None else mapped_out
        if buf.dtype != np.uint8 or not buf.flags.c_contiguous or not buf.flags.writeable:
            raise ValueError("mapped_out: a writeable contiguous uint8 array")
        mp = _lib.MemMapping()
        self._ck(lib.pgrc_mem_mark_and_remove(self._h, C.cast(mt.ctypes.data_as(C.c_void_p), C.POINTER(_lib.TextMatch)), mt.shape[0],
                                              UINT32_MAX if minMatchLength is None else int(minMatchLength),
                                              buf.ctypes.data_as(C.c_void_p), buf.size if n2 else 0, C.byref(mp)))
        off = np.ctypeslib.as_array(mp.map_off, shape=(mp.map_off_bytes,)).copy() if mp.map_off_bytes else np.zeros(0, np.uint8)
        lens = np.ctypeslib.as_array(mp.map_len, shape=(mp.map_len_bytes,)).copy()
        info = {"marks": mp.marks, "unique_matches": mp.unique_matches, "matched_symbols": mp.matched_symbols}
        mapped = buf[:mp.mapped_len]
        lib.pgrc_mem_free_mapping(C.byref(mp))
        return mapped, off, lens, info

    def markAndRemoveExactMatchesResident(self, matches, part: int, minMatchLength: int | None = None):
        """markAndRemoveExactMatches with the mapped text kept on the device, in slot `part` (0 HQ, 1 LQ, 2 N), for
        encodeMapped.  -> (mapped_len, map_off, map_len, info)"""
        mt = np.ascontiguousarray(np.asarray(matches, dtype=np.uint64).reshape(-1, 3))
        mp = _lib.MemMapping()
        self._ck(lib.pgrc_mem_mark_and_remove_resident(self._h, C.cast(mt.ctypes.data_as(C.c_void_p), C.POINTER(_lib.TextMatch)), mt.shape[0],
                                                       UINT32_MAX if minMatchLength is None else int(minMatchLength), int(part), C.byref(mp)))
        off = np.ctypeslib.as_array(mp.map_off, shape=(mp.map_off_bytes,)).copy() if mp.map_off_bytes else np.zeros(0, np.uint8)
        lens = np.ctypeslib.as_array(mp.map_len, shape=(mp.map_len_bytes,)).copy()
        info = {"marks": mp.marks, "unique_matches": mp.unique_matches, "matched_symbols": mp.matched_symbols}
        mapped_len = int(mp.mapped_len)
        self._res_len[int(part)] = mapped_len
        lib.pgrc_mem_free_mapping(C.byref(mp))
        return mapped_len, off, lens, info

    def encodeMapped(self, coder, out: np.ndarray | None = None):
        """the resident mapped texts HQ | LQ | N coded as one text by `coder` (pgrc_amd.VarLenDNACoder): what
        SimplePgMatcher::matchPgsInPg hands to LZMA / PPMd.  -> (coded, (hq_len, lq_len, n_len)); out: a uint8 buffer to
        write into (page-locked memory copies faster), else one of the worst-case size is made."""
        n = C.c_uint64(0)
        lens = (C.c_uint64 * 3)()
        if out is None:                                         # (pgrc_varlen_bound: one code a symbol at worst)
            out = np.empty(max(int(lib.pgrc_varlen_bound(sum(self._res_len))), 1), dtype=np.uint8)
        if out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError("out: a writeable contiguous uint8 array")
        self._ck(lib.pgrc_mem_encode_mapped(self._h, coder._h, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n), C.byref(lens)))
        return out[:n.value], tuple(int(x) for x in lens)

    def mapping_timing(self) -> dict:
        """phases of the last markAndRemoveExactMatches in milliseconds (introspection: tests, tools)"""
        ms = (C.c_float * 5)()
        self._ck(lib.pgrc_mem_mapping_timing(self._h, C.byref(ms)))
        return dict(zip(("ms_sort", "ms_path", "ms_streams", "ms_text", "ms_download"), (float(x) for x in ms)))

    def counters(self) -> dict:
        c = _lib.MemCounters()
        self._ck(lib.pgrc_mem_get_counters(self._h, C.byref(c)))
        return {k: getattr(c, k) for k, _ in c._fields_}

    def close(self) -> None:
        if self._h:
            lib.pgrc_mem_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
