"""Host-side mirror of the assembly of a pseudogenome from the overlap graph (include/pgrc_assemble.h): what the
reference's generator does after findOverlappingReads -- removeCyclesAndPrepareComponents, countPseudoGenomeLength,
assemblePseudoGenomeTemplate, applyIndexesMapping -- on the MI355X.  numpy in and out; no compute here."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import PgrcMatchError, lib


def row_bytes(read_len: int, symbols: int) -> int:
    """PackedConstantLengthReadsSet::packedLength"""
    return (read_len + 3) // 4 if symbols == 4 else (read_len + 2) // 3


class PgAssembler:
    def __init__(self, device: int = -1):
        self._h = C.c_void_p()
        rc = lib.pgrc_asm_create(int(device), C.byref(self._h))
        if rc:
            raise PgrcMatchError(rc, (lib.pgrc_asm_last_error(None) or b"").decode())
        self.pg_len = 0

    def _ck(self, rc: int) -> None:
        if rc:
            raise PgrcMatchError(rc, (lib.pgrc_asm_last_error(self._h) or b"").decode())

    def run(self, packed_rows, next_read, overlap, read_len: int, symbols: int = 4, index_mapping=None) -> dict:
        """packed_rows: uint8 [R, row_bytes]; next_read: uint32 [R + 1]; overlap: uint8 or uint16 [R + 1] (element 0 of both
        is ignored); index_mapping: uint32 [R] or None.
        -> org_idx (uint32 [R]), off (uint16 [R]), pg_len, cycles, overlap_lost, components, singles; the text stays on
        the device (text(), text_device(), packed_device())."""
        rows = np.ascontiguousarray(packed_rows, dtype=np.uint8)
        nx = np.ascontiguousarray(next_read, dtype=np.uint32)
        ov = np.ascontiguousarray(overlap)
        if ov.dtype not in (np.uint8, np.uint16):
            raise ValueError("overlap: uint8 or uint16")
        R = nx.size - 1
        if ov.size != nx.size or rows.size != max(R, 0) * row_bytes(read_len, symbols):
            raise ValueError("packed_rows, next_read and overlap do not describe the same reads")
        mp = None if index_mapping is None else np.ascontiguousarray(index_mapping, dtype=np.uint32)
        if mp is not None and mp.size != R:
            raise ValueError("index_mapping: one entry per read")
        inp = _lib.AsmInput(C.sizeof(_lib.AsmInput), int(read_len), int(symbols), ov.dtype.itemsize, max(R, 0),
                            rows.ctypes.data_as(C.c_void_p), nx.ctypes.data_as(C.c_void_p), ov.ctypes.data_as(C.c_void_p),
                            None if mp is None else mp.ctypes.data_as(C.c_void_p))
        res = _lib.AsmResult()
        self.pg_len = 0
        self._ck(lib.pgrc_asm_run(self._h, C.byref(inp), C.byref(res)))
        n = res.n_reads
        out = {"org_idx": np.ctypeslib.as_array(res.org_idx, shape=(n,)).copy(), "off": np.ctypeslib.as_array(res.off, shape=(n,)).copy(),
               "pg_len": res.pg_len, "cycles": res.cycles, "overlap_lost": res.overlap_lost, "components": res.components,
               "singles": res.singles}
        self.pg_len = res.pg_len
        lib.pgrc_asm_free_result(C.byref(res))
        return out

    def text(self, first: int = 0, n: int | None = None, out: np.ndarray | None = None) -> np.ndarray:
        """n bytes of the ASCII text from `first` on (all of it by default) as uint8"""
        n = self.pg_len - first if n is None else n
        buf = np.empty(max(n, 0), dtype=np.uint8) if out is None else out
        self._ck(lib.pgrc_asm_get_text(self._h, int(first), int(n), buf.ctypes.data_as(C.c_void_p)))
        return buf[:n]

    def text_device(self) -> tuple[int, int]:
        """-> (device address of the ASCII text, its length); valid until the next run"""
        p, n = C.c_void_p(), C.c_uint64(0)
        self._ck(lib.pgrc_asm_text_device(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def packed_device(self) -> int:
        """-> device address of the text at 2 bits per symbol, as pgrc_match_set_pg_packed_device takes it (ACGT only)"""
        p = C.c_void_p()
        self._ck(lib.pgrc_asm_packed_device(self._h, C.byref(p)))
        return p.value

    def timing(self) -> dict:
        t = _lib.AsmTiming(C.sizeof(_lib.AsmTiming))
        self._ck(lib.pgrc_asm_get_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_ if k != "struct_size"}

    def close(self) -> None:
        if self._h:
            lib.pgrc_asm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
