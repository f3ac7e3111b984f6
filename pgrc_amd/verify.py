"""Host-side mirror of include/pgrc_verify.h: does a decode job give its source reads back?  The rows are rebuilt, keyed,
sorted and compared on the MI355X; only counters come back.  No compute here.

    dec = PgRCDecoder(L); dec.set_text(...); dec.add_list(...); dec.set_order(...)
    with dec.verifier() as v:                # IN_ORDER for an ORD job, MULTISET for SE and PE
        v.add_rows(0, source_rows)           # or v.add_fastq(text[, pair_text], final=True)
        res = v.finish()                     # res["ok"]
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import PgrcMatchError, VerifyResult, VerifyTiming

_P = C.c_void_p

VERIFY_AUTO, VERIFY_IN_ORDER, VERIFY_MULTISET = 0, 1, 2
VERIFY_MAX_ITEMS = 0x7FFFF800
NONE64, NONE32 = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF


def _u8(a) -> np.ndarray:
    if isinstance(a, str):
        a = a.encode("latin-1")
    if isinstance(a, (bytes, bytearray, memoryview)):
        return np.frombuffer(a, dtype=np.uint8)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Verifier:
    """One verification of `decoder`'s job (text, lists and order set).  Keeps the decoder alive; the decoder's job must
    not change until close()."""

    def __init__(self, decoder, kind: int = VERIFY_AUTO, library=None):
        self._lib = _lib.vlib if library is None else library     # (tests: another library that holds pgrc_verify_*)
        self._h = _P()
        self.decoder = decoder
        self.readLength = int(decoder.readLength)
        rc = self._lib.pgrc_verify_begin(decoder._h, int(kind), C.byref(self._h))
        if rc:
            raise PgrcMatchError(rc, (self._lib.pgrc_verify_last_error(None) or b"").decode())

    def _ck(self, rc: int) -> None:
        if rc:
            raise PgrcMatchError(rc, (self._lib.pgrc_verify_last_error(self._h) or b"").decode())

    def add_rows(self, file: int, rows, n: int | None = None) -> None:
        """source rows of `file`, in source order: a uint8 array of shape (n, L), bytes of n * L symbols, or (with n given)
        the address of n rows in host memory, page-locked or not"""
        if isinstance(rows, int):
            self._ck(self._lib.pgrc_verify_add_rows(self._h, int(file), _P(rows), int(n)))
            return
        a = _u8(rows)
        assert a.size % self.readLength == 0, "rows of the read length, without newlines"
        self._ck(self._lib.pgrc_verify_add_rows(self._h, int(file), a.ctypes.data_as(_P) if a.size else None, a.size // self.readLength))

    def add_fastq(self, text, pair_text=None, final: bool | int = False):
        """a piece of the source's FASTQ text (and of its pair file); -> (consumed, pair_consumed, records taken).  The
        caller hands the rest of each piece over again in front of what it reads next.  final: True where nothing follows
        in either file, or pgrc_divider_run_fastq's final_piece bits"""
        t = _u8(text)
        p = None if pair_text is None else _u8(pair_text)
        used, pused, nrec = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        fin = int(final) if not isinstance(final, bool) else (1 if final else 0)
        # (an empty piece of the pair file is still a pair file: a non-NULL pointer with no byte)
        keep = np.zeros(1, np.uint8)
        self._ck(self._lib.pgrc_verify_add_fastq(self._h, t.ctypes.data_as(_P) if t.size else None, t.size,
                                                 None if p is None else (p if p.size else keep).ctypes.data_as(_P), 0 if p is None else p.size,
                                                 fin, C.byref(used), C.byref(pused) if p is not None else None, C.byref(nrec)))
        return used.value, pused.value, nrec.value

    def add_text(self, fmt, text, pair_text=None, final: bool | int = False):
        """add_fastq for any of the reference's three text formats (pgrc_verify_add_text, include/pgrc_reads_text.h): fmt is
        "fastq", "fasta" or "lines", or a PGRC_READS_* number"""
        t = _u8(text)
        p = None if pair_text is None else _u8(pair_text)
        used, pused, nrec = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        fin = int(final) if not isinstance(final, bool) else (1 if final else 0)
        keep = np.zeros(1, np.uint8)
        # (libpgrc_reads_text.so holds the verifier's code too: a handle of either library is a handle of the other)
        rc = _lib.tlib.pgrc_verify_add_text(self._h, _lib.reads_format(fmt), t.ctypes.data_as(_P) if t.size else None, t.size,
                                            None if p is None else (p if p.size else keep).ctypes.data_as(_P), 0 if p is None else p.size,
                                            fin, C.byref(used), C.byref(pused) if p is not None else None, C.byref(nrec))
        self._ck(rc)
        return used.value, pused.value, nrec.value

    def finish(self) -> dict:
        """the result, once: pgrc_verify_result's fields by name (n_source and n_decoded as lists, ok as a bool)"""
        r = VerifyResult()
        r.struct_size = C.sizeof(VerifyResult)
        self._ck(self._lib.pgrc_verify_finish(self._h, C.byref(r)))
        d = {k: getattr(r, k) for k, _ in r._fields_ if k != "struct_size"}
        d["n_source"], d["n_decoded"], d["ok"] = list(r.n_source), list(r.n_decoded), bool(r.ok)
        return d

    def timing(self) -> dict:
        t = VerifyTiming()
        t.struct_size = C.sizeof(VerifyTiming)
        self._ck(self._lib.pgrc_verify_get_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_ if k != "struct_size"}

    def close(self) -> None:
        if self._h:
            self._lib.pgrc_verify_end(self._h)
            self._h = _P()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
