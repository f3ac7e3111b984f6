"""Host-side mirror of the overlap search of the pseudogenome generator (include/pgrc_overlap.h): what the reference's
GreedySwipingPackedOverlapGeneratorTemplate::findOverlappingReads does at one thread -- the duplicates' chains and the sweeps
that link a read's suffix to another read's prefix -- or, under rule="parallel", what the parallel generator's does, and
getBothSidesOverlappedReads, on the MI355X.  numpy in and out; no compute here."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import PgrcMatchError, lib
from .assemble import PgAssembler, row_bytes


class OverlapFinder:
    def __init__(self, device: int = -1):
        self._h = C.c_void_p()
        rc = lib.pgrc_ovl_create(int(device), C.byref(self._h))
        if rc:
            raise PgrcMatchError(rc, (lib.pgrc_ovl_last_error(None) or b"").decode())
        self.n_reads = 0
        self.sweeps = 0

    def _ck(self, rc: int) -> None:
        if rc:
            raise PgrcMatchError(rc, (lib.pgrc_ovl_last_error(self._h) or b"").decode())

    def set_rule(self, rule: str) -> None:
        """the rule of the later runs: "serial" (the generator of one thread) or "parallel" (the parallel generator)"""
        if rule not in _lib.OVL_RULES:
            raise ValueError('rule: "serial" or "parallel"')
        self._ck(lib.pgrc_ovlrule_set(self._h, _lib.OVL_RULES[rule]))

    def rule_info(self) -> dict:
        """pgrc_ovl_rule_info of the last run: rule ("serial" | "parallel"), blocks, tail_sweeps, follower_compares,
        past_end_compares"""
        info = _lib.OvlRuleInfo(C.sizeof(_lib.OvlRuleInfo))
        self._ck(lib.pgrc_ovlrule_get_info(self._h, C.byref(info)))
        out = {k: int(getattr(info, k)) for k, _ in info._fields_ if k != "struct_size"}
        out["rule"] = {v: k for k, v in _lib.OVL_RULES.items()}[out["rule"]]
        return out

    def run(self, packed_rows, read_len: int, symbols: int = 4, stop_coef: float = 1.0, sorted_order=None, overlap_width: int = 1,
            rule: str | None = None) -> dict:
        """packed_rows: uint8 [R, row_bytes]; sorted_order: the read numbers 1 .. R in sorted order (uint32 [R]) or None: made
        on the device, equal reads in ascending number; rule: "serial" | "parallel", kept for the later runs (None: as it is).
        -> next_read (uint32 [R + 1]), overlap (uint8 or uint16 [R + 1]), reads_left (uint64: after the duplicates, then after
        every sweep), duplicates, links, sweeps; rows and graph stay on the device (both_sides(), assemble())."""
        if rule is not None:
            self.set_rule(rule)
        rows = np.ascontiguousarray(packed_rows, dtype=np.uint8)
        rb = row_bytes(read_len, symbols)
        R = rows.size // rb if rb else 0
        if rows.size != R * rb:
            raise ValueError("packed_rows: whole rows of row_bytes(read_len, symbols) bytes")
        so = None if sorted_order is None else np.ascontiguousarray(sorted_order, dtype=np.uint32)
        if so is not None and so.size != R:
            raise ValueError("sorted_order: one entry per read")
        inp = _lib.OvlInput(C.sizeof(_lib.OvlInput), int(read_len), int(symbols), int(overlap_width), R, float(stop_coef),
                            rows.ctypes.data_as(C.c_void_p), None if so is None else so.ctypes.data_as(C.c_void_p))
        res = _lib.OvlResult()
        self.n_reads = 0
        self._ck(lib.pgrc_ovl_run(self._h, C.byref(inp), C.byref(res)))
        n = res.n_reads + 1
        ov_t = C.c_uint8 if overlap_width == 1 else C.c_uint16
        out = {"next_read": np.ctypeslib.as_array(res.next_read, shape=(n,)).copy(),
               "overlap": np.ctypeslib.as_array(C.cast(res.overlap, C.POINTER(ov_t)), shape=(n,)).copy(),
               "reads_left": np.ctypeslib.as_array(res.reads_left_after, shape=(res.n_left,)).copy(),
               "duplicates": res.duplicates, "links": res.links, "sweeps": res.sweeps}
        self.n_reads = res.n_reads
        self.sweeps = res.sweeps
        lib.pgrc_ovl_free_result(C.byref(res))
        return out

    def both_sides(self) -> np.ndarray:
        """getBothSidesOverlappedReads of the last run: uint8 [R]"""
        flags = np.empty(max(self.n_reads, 1), dtype=np.uint8)
        self._ck(lib.pgrc_ovl_both_sides(self._h, flags.ctypes.data_as(C.c_void_p)))
        return flags[:self.n_reads]

    def assemble(self, assembler: PgAssembler, index_mapping=None) -> dict:
        """PgAssembler.run on the last run's rows and graph, handed over on the device -> as PgAssembler.run"""
        mp = None if index_mapping is None else np.ascontiguousarray(index_mapping, dtype=np.uint32)
        if mp is not None and mp.size != self.n_reads:
            raise ValueError("index_mapping: one entry per read")
        res = _lib.AsmResult()
        assembler.pg_len = 0
        self._ck(lib.pgrc_ovl_assemble(self._h, assembler._h, None if mp is None else mp.ctypes.data_as(C.c_void_p), C.byref(res)))
        n = res.n_reads
        out = {"org_idx": np.ctypeslib.as_array(res.org_idx, shape=(n,)).copy(), "off": np.ctypeslib.as_array(res.off, shape=(n,)).copy(),
               "pg_len": res.pg_len, "cycles": res.cycles, "overlap_lost": res.overlap_lost, "components": res.components,
               "singles": res.singles}
        assembler.pg_len = res.pg_len
        lib.pgrc_asm_free_result(C.byref(res))
        return out

    def timing(self) -> dict:
        t = _lib.OvlTiming(C.sizeof(_lib.OvlTiming))
        self._ck(lib.pgrc_ovl_get_timing(self._h, C.byref(t)))
        out = {k: getattr(t, k) for k, _ in t._fields_ if k != "struct_size"}
        ms = (C.c_float * max(self.sweeps, 1))()
        self._ck(lib.pgrc_ovl_get_sweep_ms(self._h, ms, self.sweeps))
        out["ms_sweeps_device"] = [float(x) for x in ms[:self.sweeps]]
        return out

    def close(self) -> None:
        if self._h:
            lib.pgrc_ovl_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
