"""A pseudogenome's reads list on the device from the assembly to the archive (include/pgrc_readslist.h, and
include/pgrc_readslist_ord.h for the order-preserving mode, whose four calls libpgrc_rlist_ord.so exports): ReadsList mirrors
the calls.  No compute of its own."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._lib import PgrcMatchError, lib, olib
from .decode import PairOrderStreams, PairPosStreams, _list_archive_dict, _pairorder_dict, _pairpos_dict
from .matchers import MatchContext


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


class ReadsList:
    """off, orgIdx, revComp and the mismatch streams of one pseudogenome's reads list in device memory.  Producers: set_host,
    from_assembly, export_pg_order, export_original_order; consumers: download, archive_encode, archive_encode_ord, pair_order,
    pair_positions, positions."""

    def __init__(self, device: int = -1):
        self._h = C.c_void_p()
        code = lib.pgrc_rlist_create(int(device), C.byref(self._h))
        if code:
            raise PgrcMatchError(code, (lib.pgrc_rlist_last_error(None) or b"").decode())

    def _ck(self, code: int) -> None:
        if code:
            raise PgrcMatchError(code, (lib.pgrc_rlist_last_error(self._h) or b"").decode())

    def info(self) -> dict:
        i = _lib.RlistInfo(C.sizeof(_lib.RlistInfo))
        self._ck(lib.pgrc_rlist_get_info(self._h, C.byref(i)))
        return {"off_width": int(i.off_width), "n_entries": int(i.n_entries), "n_mismatches": int(i.n_mismatches), "last_pos": int(i.last_pos),
                "has_rev_comp": bool(i.has_rev_comp), "has_mismatches": bool(i.has_mismatches)}

    def timing(self) -> dict:
        t = _lib.RlistTiming(C.sizeof(_lib.RlistTiming))
        self._ck(lib.pgrc_rlist_get_timing(self._h, C.byref(t)))
        out = {k: getattr(t, k) for k, _ in t._fields_ if k != "struct_size"}
        out["call"] = _lib.RLIST_CALLS.get(int(t.call), "?")
        return out

    def set_host(self, off, org_idx, rev_comp=None, mis_cnt=None, mis_sym=None, mis_rev_off=None, last_pos: int = 0,
                 n_mismatches: Optional[int] = None) -> None:
        """the list from host arrays; off's dtype (uint8 or uint16) is the list's off_width.  n_mismatches: what the caller
        claims (default: mis_sym's size)"""
        off = np.ascontiguousarray(off)
        assert off.dtype in (np.uint8, np.uint16)
        ot = off.dtype
        keep = [off, np.ascontiguousarray(org_idx, dtype=np.uint32)]
        st = _lib.ExportStreams()
        st.n_entries, st.off_width, st.last_pos = keep[1].size, ot.itemsize, int(last_pos)
        st.off = C.cast(_p(off), C.POINTER(C.c_uint8))
        st.org_idx = C.cast(_p(keep[1]), C.POINTER(C.c_uint32))
        for name, a, dt in (("rev_comp", rev_comp, np.uint8), ("mis_cnt", mis_cnt, np.uint8), ("mis_sym", mis_sym, np.uint8), ("mis_rev_off", mis_rev_off, ot)):
            if a is None:
                continue
            a = np.ascontiguousarray(a, dtype=dt)
            if not a.size:
                a = np.zeros(1, dtype=dt)           # an empty stream is present too: something to point at
            keep.append(a)
            setattr(st, name, C.cast(a.ctypes.data_as(C.c_void_p), C.POINTER(C.c_uint8)))
        st.n_mismatches = int(n_mismatches) if n_mismatches is not None else (0 if mis_sym is None else np.asarray(mis_sym).size)
        self._ck(lib.pgrc_rlist_set_host(self._h, C.byref(st)))

    def from_assembly(self, assembler, sets=None, which="hq") -> None:
        """the list of the assembler's last run (PgAssembler, or anything with the context in _h), the indexes mapped through
        the read sets' mapping `which` on the device"""
        w = _lib.RSETS_WHICH[which] if isinstance(which, str) else int(which)
        self._ck(lib.pgrc_rlist_from_assembly(self._h, assembler._h, sets._h if sets is not None else None, w))

    def from_overlap(self, finder, assembler, sets=None, which="hq") -> dict:
        """OverlapFinder.assemble without an index mapping and from_assembly in one call, the assembly's copy of the reads
        list to the host left out -> pg_len, cycles, overlap_lost, components, singles"""
        w = _lib.RSETS_WHICH[which] if isinstance(which, str) else int(which)
        res = _lib.AsmResult()
        assembler.pg_len = 0
        self._ck(lib.pgrc_rlist_from_overlap(self._h, finder._h, assembler._h, sets._h if sets is not None else None, w, C.byref(res)))
        assembler.pg_len = res.pg_len
        return {k: getattr(res, k) for k in ("pg_len", "cycles", "overlap_lost", "components", "singles")}

    def export_pg_order(self, matcher, order=None, read_org_idx=None, sets=None, rev_compl_pair_file: bool = False,
                        byte_per_read_length: bool = True) -> None:
        """exportMatchesInPgOrder with this list as the old one; the merged list replaces it.  order=None: made on the device"""
        a = _lib.RlistExportArgs(C.sizeof(_lib.RlistExportArgs))
        keep = []
        if order is None:
            a.order_on_device = 1
        else:
            keep.append(np.ascontiguousarray(order, dtype=np.uint32))
            a.order, a.n_matched = (keep[-1].ctypes.data if keep[-1].size else None), keep[-1].size
        if read_org_idx is not None:
            keep.append(np.ascontiguousarray(read_org_idx, dtype=np.uint32))
            a.read_org_idx = keep[-1].ctypes.data
        if sets is not None:
            a.sets = sets._h
        a.rev_compl_pair_file, a.byte_per_read_length = int(rev_compl_pair_file), int(byte_per_read_length)
        self._ck(lib.pgrc_rlist_export_pg_order(self._h, matcher._h, C.byref(a)))

    def export_original_order(self, matcher, total: int, read_org_idx=None, sets=None, pair_file_mode: bool = False,
                              rev_compl_pair_file: bool = False, byte_per_read_length: bool = True) -> None:
        """exportMatchesInOriginalOrder: one entry per original index below `total`; the result replaces this list"""
        a = _lib.RlistExportOrgArgs(C.sizeof(_lib.RlistExportOrgArgs))
        keep = None
        if read_org_idx is not None:
            keep = np.ascontiguousarray(read_org_idx, dtype=np.uint32)
            a.read_org_idx = keep.ctypes.data
        if sets is not None:
            a.sets = sets._h
        a.reads_total_count, a.pair_file_mode = int(total), int(pair_file_mode)
        a.rev_compl_pair_file, a.byte_per_read_length = int(rev_compl_pair_file), int(byte_per_read_length)
        self._ck(olib.pgrc_rlist_export_original_order(self._h, matcher._h, C.byref(a)))

    def download(self) -> dict:
        """the streams as MatchContext.export_pg_order returns them"""
        st = _lib.ExportStreams()
        self._ck(lib.pgrc_rlist_download(self._h, C.byref(st)))
        return MatchContext._streams(st)

    def archive_encode(self, fast_level: bool = False, want_org_idx: bool = False) -> dict:
        """what compressedBuild hands to the coders: off, rev_comp (None: the list has none), org_idx (None: not asked for),
        archive (as PgRCDecoder.list_archive_encode returns it; None for a list without mismatch streams), block_bytes"""
        a = _lib.RlistArchive()
        self._ck(lib.pgrc_rlist_archive_encode(self._h, int(bool(fast_level)), int(bool(want_org_idx)), C.byref(a)))
        return self._archive_dict(a)

    def archive_encode_ord(self, fast_level: bool = False) -> dict:
        """what compressedBuild(.., ignoreOffDest = true) hands to the coders in the order-preserving mode: as archive_encode
        returns it, with off and org_idx None (the block holds neither) and block_start = "rev_comp", the stream at the start
        of the block"""
        a = _lib.RlistArchive()
        self._ck(olib.pgrc_rlist_archive_encode_ord(self._h, int(bool(fast_level)), C.byref(a)))
        start = "rev_comp" if a.rev_comp and a.rev_comp == a.block else None
        return dict(self._archive_dict(a), block_start=start)

    @staticmethod
    def _archive_dict(a) -> dict:
        try:
            n, w = int(a.n_entries), int(a.off_width)

            def take(p, count, dt):
                dt = np.dtype(dt)
                return np.frombuffer((C.c_uint8 * (count * dt.itemsize)).from_address(p), dtype=dt).copy() if count else np.zeros(0, dt)
            out = {"n_entries": n, "off_width": w, "block_bytes": int(a.block_bytes),
                   "off": take(a.off, n, np.uint8 if w == 1 else np.uint16) if a.off else None,
                   "rev_comp": take(a.rev_comp, n, np.uint8) if a.rev_comp else None,
                   "org_idx": take(a.org_idx, n, np.uint32) if a.org_idx else None,
                   "archive": _list_archive_dict(a.archive, a.block) if a.archive.struct_size else None}
            end = a.block + int(a.block_bytes)
            out["one_block"] = all(p is None or a.block <= p <= end for p in (a.off, a.rev_comp, a.org_idx, a.archive.zero_flags, a.archive.nonzero_cnt))
        finally:
            lib.pgrc_rlist_archive_free(C.byref(a))
        return out

    @staticmethod
    def pair_order(lists, form: int) -> dict:
        """compressReadsOrder over the lists HQ, LQ, N (None: no such list) -> as PgRCDecoder.compressReadsOrder"""
        lists = list(lists) + [None] * (3 - len(lists))
        h = (C.c_void_p * 3)(*[l._h if l is not None else None for l in lists])
        first = next((l for l in lists if l is not None), None)
        s = PairOrderStreams()
        code = lib.pgrc_rlist_pair_order(h, int(form), C.byref(s))
        if code:
            raise PgrcMatchError(code, (lib.pgrc_rlist_last_error(first._h) or b"").decode() if first is not None else "no list")
        try:
            return _pairorder_dict(s)
        finally:
            lib.pgrc_pairorder_free(C.byref(s))

    def _pairpos_args(self, n_total, pos_width, lq, n, hq_len, lq_len, matcher, read_org_idx, sets):
        a = _lib.RlistPairPosArgs(C.sizeof(_lib.RlistPairPosArgs), int(pos_width), int(n_total))
        a.hq, a.lq, a.n = self._h, (lq._h if lq is not None else None), (n._h if n is not None else None)
        a.hq_len, a.lq_len = int(hq_len), int(lq_len)
        keep = None
        if matcher is not None:
            a.matcher = matcher._h
        if read_org_idx is not None:
            keep = np.ascontiguousarray(read_org_idx, dtype=np.uint32)
            a.read_org_idx = keep.ctypes.data
        if sets is not None:
            a.sets = sets._h
        return a, keep

    def pair_positions(self, n_total: int, pos_width: int, lq=None, n=None, hq_len: int = 0, lq_len: int = 0, matcher=None,
                       read_org_idx=None, sets=None) -> dict:
        """orgIdx2PgPos of the order-preserving paired mode from this (HQ) list, the LQ and N lists and the matcher's matched
        reads, built and coded on the device -> as PgRCDecoder.compressReadsPgPositions"""
        a, keep = self._pairpos_args(n_total, pos_width, lq, n, hq_len, lq_len, matcher, read_org_idx, sets)
        s = PairPosStreams()
        self._ck(lib.pgrc_rlist_pair_positions(C.byref(a), C.byref(s)))
        try:
            return _pairpos_dict(s)
        finally:
            lib.pgrc_pairpos_free(C.byref(s))

    def positions(self, n_total: int, pos_width: int, lq=None, n=None, hq_len: int = 0, lq_len: int = 0, matcher=None,
                  read_org_idx=None, sets=None) -> np.ndarray:
        """orgIdx2PgPos of the order-preserving single-file mode, built as pair_positions builds it (n_total may be odd) and
        narrowed to pos_width bytes on the device -> n_total positions, uint32 or uint64"""
        a, keep = self._pairpos_args(n_total, pos_width, lq, n, hq_len, lq_len, matcher, read_org_idx, sets)
        o = _lib.RlistPositionsOut(C.sizeof(_lib.RlistPositionsOut))
        self._ck(olib.pgrc_rlist_positions(C.byref(a), C.byref(o)))
        try:
            dt = np.dtype(np.uint32 if int(o.pos_width) == 4 else np.uint64)
            T = int(o.n_total)
            assert o.positions == o.block and int(o.block_bytes) == T * dt.itemsize
            return np.frombuffer((C.c_uint8 * (T * dt.itemsize)).from_address(o.positions), dtype=dt).copy() if T else np.zeros(0, dt)
        finally:
            olib.pgrc_rlist_positions_free(C.byref(o))

    def close(self) -> None:
        if self._h:
            lib.pgrc_rlist_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
