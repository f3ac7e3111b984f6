"""Host-side mirror of the reference's read-set division (readsset/DividedPCLReadsSets.h) on top of
include/pgrc_reads.h, and of the divided sets kept on the device between the encoder's stages (include/pgrc_readsets.h):
computes nothing itself."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._lib import PgrcMatchError, lib


def reads_text_format(first_byte) -> int:
    """the reference's choice of the reads source by the first byte of the file (pgrc_reads_text_format): a byte value, a
    bytes object (its first byte; empty: -1, the end of the file) or -1 -> 0 FASTQ, 1 FASTA, 2 one read per line"""
    if isinstance(first_byte, (bytes, bytearray)):
        first_byte = first_byte[0] if len(first_byte) else -1
    return int(_lib.tlib.pgrc_reads_text_format(int(first_byte)))


class DividedPCLReadsSets:
    """DividedPCLReadsSets::getQualityDivisionBasedReadsSets (DividedPCLReadsSets.cpp:59-100) over batches of FASTQ
    records given as row arrays.  `divide(reads, quals)` returns the packed rows of the HQ / LQ / N sets of the batch
    (PackedConstantLengthReadsSet::packedReads layout) and the batch-local indexes of the LQ / N reads."""

    def __init__(self, readLength: int, error_limit: float = 1.0, simplified_suffix_mode: bool = True,
                 separateNReadsSet: bool = False, nReadsLQ: bool = False, device: int = -1):
        prm = _lib.DivideParams(int(readLength), float(error_limit), int(bool(simplified_suffix_mode)),
                                int(bool(separateNReadsSet)), int(bool(nReadsLQ)), int(device))
        self._h = C.c_void_p()
        code = lib.pgrc_divider_create(C.byref(prm), C.byref(self._h))
        if code:
            raise PgrcMatchError(code, (lib.pgrc_divider_last_error(None) or b"").decode())
        self.readLength = int(readLength)
        self.needs_quality = error_limit < 1

    def _ck(self, code: int) -> None:
        if code:
            raise PgrcMatchError(code, (lib.pgrc_divider_last_error(self._h) or b"").decode())

    def divide(self, reads: np.ndarray, quals: Optional[np.ndarray] = None) -> dict:
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        n = reads.shape[0] if reads.ndim == 2 else reads.size // self.readLength
        assert reads.size == n * self.readLength
        qp = None
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
            assert quals.size == reads.size
            qp = quals.ctypes.data_as(C.c_void_p)
        out = _lib.DividedReads()
        self._ck(lib.pgrc_divider_run(self._h, reads.ctypes.data_as(C.c_void_p), qp, n, C.byref(out)))
        return self._result(out)

    def _result(self, out) -> dict:
        def arr(ptr, count, dtype):
            if not count:
                return np.zeros(0, dtype=dtype)
            a = np.empty(count, dtype=dtype)                 # (the library's arrays live until the next run: copy out)
            C.memmove(a.ctypes.data, ptr, a.nbytes)
            return a
        return {"n_hq": int(out.n_hq), "n_lq": int(out.n_lq), "n_n": int(out.n_n),
                "symbols": (int(out.hq_symbols), int(out.lq_symbols), int(out.n_symbols)),
                "row_bytes": (int(out.hq_row_bytes), int(out.lq_row_bytes), int(out.n_row_bytes)),
                "hq_rows": arr(out.hq_rows, out.n_hq * out.hq_row_bytes, np.uint8),
                "lq_rows": arr(out.lq_rows, out.n_lq * out.lq_row_bytes, np.uint8),
                "n_rows": arr(out.n_rows, out.n_n * out.n_row_bytes, np.uint8),
                "lq_index": arr(out.lq_index, out.n_lq, np.uint32), "n_index": arr(out.n_index, out.n_n, np.uint32)}

    def _run_text(self, run, text: bytes, pair_text: Optional[bytes], rev_compl_pair: bool, final):
        """run(text, bytes, pair_text, pair_bytes, rev_compl_pair, final_piece, consumed, pair_consumed, n_records, out) -> what
        divide_fastq returns"""
        out = _lib.DividedReads()
        used, pused, nrec = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        t = np.frombuffer(text, dtype=np.uint8) if len(text) else np.zeros(1, np.uint8)
        pt = None
        if pair_text is not None:
            pt = np.frombuffer(pair_text, dtype=np.uint8) if len(pair_text) else np.zeros(1, np.uint8)
        self._ck(run(t.ctypes.data_as(C.c_void_p), len(text), pt.ctypes.data_as(C.c_void_p) if pt is not None else None,
                     len(pair_text) if pair_text is not None else 0, int(bool(rev_compl_pair)), int(final),
                     C.byref(used), C.byref(pused), C.byref(nrec), C.byref(out)))
        return self._result(out), int(nrec.value), int(used.value), int(pused.value)

    def divide_fastq(self, text: bytes, pair_text: Optional[bytes] = None, rev_compl_pair: bool = False, final=True):
        """One piece of FASTQ text (and of the pair file's): (result dict, records taken, bytes consumed, pair bytes consumed).
        final: True / 1 = nothing follows in either text; 2 / 4 = only the first / the second text ends here."""
        return self._run_text(lambda *a: lib.pgrc_divider_run_fastq(self._h, *a), text, pair_text, rev_compl_pair, final)

    def divide_text(self, fmt, text: bytes, pair_text: Optional[bytes] = None, rev_compl_pair: bool = False, final=True):
        """divide_fastq for any of the reference's three text formats (pgrc_divider_run_text): fmt is "fastq", "fasta" or
        "lines" (one read per line), or what reads_text_format gives for the file's first byte.  Returns what divide_fastq
        returns."""
        fmt = _lib.reads_format(fmt)
        return self._run_text(lambda *a: lib.pgrc_divider_run_text(self._h, fmt, *a), text, pair_text, rev_compl_pair, final)

    def last_was_terminal(self) -> bool:
        """did the last divide_fastq / divide_text take the last records the reference's iteration would take (pgrc_divider_last_was_terminal)"""
        return bool(lib.pgrc_divider_last_was_terminal(self._h))

    def last_ms(self):
        ms = (C.c_float * 3)()
        self._ck(lib.pgrc_divider_last_ms(self._h, C.byref(ms)))
        return {"upload": ms[0], "kernels": ms[1], "download": ms[2]}

    def close(self) -> None:
        if self._h:
            lib.pgrc_divider_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DividedReadsSets:
    """The DividedPCLReadsSets object on the device (include/pgrc_readsets.h): the packed HQ / LQ / N sets and the two index
    mappings, filled from the divider, edited where they lie (moveLqReadsFromHqReadsSetsToLqReadsSets,
    generateHqReadsIndexesMapping, removeReadsFromLqReadsSet / removeReadsFromNReadsSet) and handed to the overlap search and
    the matcher without a row or a per-read flag crossing the link.  `which` is "hq", "lq" or "n"."""

    def __init__(self, readLength: int, separateNReadsSet: bool = False, nReadsLQ: bool = False, device: int = -1):
        prm = _lib.RsetsParams(C.sizeof(_lib.RsetsParams), int(readLength), int(bool(separateNReadsSet)), int(bool(nReadsLQ)), int(device))
        self._h = C.c_void_p()
        code = lib.pgrc_rsets_create(C.byref(prm), C.byref(self._h))
        if code:
            raise PgrcMatchError(code, (lib.pgrc_rsets_last_error(None) or b"").decode())
        self.readLength = int(readLength)

    def _ck(self, code: int) -> None:
        if code:
            raise PgrcMatchError(code, (lib.pgrc_rsets_last_error(self._h) or b"").decode())

    @staticmethod
    def _which(which) -> int:
        return _lib.RSETS_WHICH[which] if isinstance(which, str) else int(which)

    def append(self, batch: dict, n_records: Optional[int] = None) -> None:
        """a batch as DividedPCLReadsSets.divide returns it"""
        keep = [np.ascontiguousarray(batch[k], dtype=np.uint8) for k in ("hq_rows", "lq_rows", "n_rows")]
        keep += [np.ascontiguousarray(batch[k], dtype=np.uint32) for k in ("lq_index", "n_index")]
        ptr = [a.ctypes.data_as(C.c_void_p) if a.size else None for a in keep]
        b = _lib.DividedReads(int(batch["n_hq"]), int(batch["n_lq"]), int(batch["n_n"]), *[int(x) for x in batch["symbols"]],
                              *[int(x) for x in batch["row_bytes"]], *ptr)
        if n_records is None:
            n_records = b.n_hq + b.n_lq + b.n_n
        self._ck(lib.pgrc_rsets_append(self._h, C.byref(b), int(n_records)))

    def append_divider(self, divider: DividedPCLReadsSets) -> None:
        """the sets of the divider's last run, copied on the device"""
        self._ck(lib.pgrc_rsets_append_divider(self._h, divider._h))

    def finish(self) -> None:
        self._ck(lib.pgrc_rsets_finish(self._h))

    def info(self) -> dict:
        i = _lib.RsetsInfo(C.sizeof(_lib.RsetsInfo))
        self._ck(lib.pgrc_rsets_get_info(self._h, C.byref(i)))
        return {"finished": bool(i.finished), "reads_total_count": int(i.reads_total_count), "count": tuple(int(x) for x in i.count),
                "symbols": tuple(int(x) for x in i.symbols), "row_bytes": tuple(int(x) for x in i.row_bytes),
                "disposed": tuple(bool(x) for x in i.disposed)}

    def get_rows(self, which, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        w = self._which(which)
        i = self.info()
        if n is None:
            n = i["count"][w] - first
        out = np.empty((max(int(n), 0), i["row_bytes"][w]), dtype=np.uint8)
        self._ck(lib.pgrc_rsets_get_rows(self._h, w, int(first), int(n), out.ctypes.data_as(C.c_void_p)))
        return out

    def get_mapping(self, which) -> np.ndarray:
        """count + 1 entries, the guard last; "hq": generateHqReadsIndexesMapping"""
        w = self._which(which)
        i = self.info()
        n = i["count"][w] if w else i["reads_total_count"] - i["count"][1] - i["count"][2]     # HQ: the indexes in neither mapping
        out = np.empty(n + 1, dtype=np.uint32)
        self._ck(lib.pgrc_rsets_get_mapping(self._h, w, out.ctypes.data_as(C.c_void_p)))
        return out

    def dispose(self, which) -> None:
        self._ck(lib.pgrc_rsets_dispose(self._h, self._which(which)))

    @staticmethod
    def _flags(flags, on_device: bool):
        if on_device:
            return C.c_void_p(int(flags)), None
        a = np.ascontiguousarray(flags, dtype=np.uint8)
        return (a.ctypes.data_as(C.c_void_p) if a.size else None), a

    def move_lq(self, is_hq, on_device: bool = False) -> None:
        """is_hq: one byte per HQ row, or (on_device) a device pointer to them"""
        p, keep = self._flags(is_hq, on_device)
        self._ck(lib.pgrc_rsets_move_lq(self._h, p, int(bool(on_device))))

    def move_by_overlap(self, finder) -> None:
        self._ck(lib.pgrc_rsets_move_by_overlap(self._h, finder._h))

    def remove(self, is_mapped, on_device: bool = False) -> None:
        """is_mapped: LQ count + N count bytes, the LQ set's first, or (on_device) a device pointer to them"""
        p, keep = self._flags(is_mapped, on_device)
        self._ck(lib.pgrc_rsets_remove(self._h, p, int(bool(on_device))))

    def remove_matched(self, matcher) -> None:
        self._ck(lib.pgrc_rsets_remove_matched(self._h, matcher._h))

    def overlap(self, which, finder, stop_coef: float = 1.0, overlap_width: int = 1, sorted_order=None) -> dict:
        """OverlapFinder.run on the set's rows, taken on the device -> as OverlapFinder.run"""
        so = None if sorted_order is None else np.ascontiguousarray(sorted_order, dtype=np.uint32)
        res = _lib.OvlResult()
        finder.n_reads = 0
        self._ck(lib.pgrc_rsets_overlap(self._h, self._which(which), finder._h, float(stop_coef), int(overlap_width),
                                        None if so is None else so.ctypes.data_as(C.c_void_p), C.byref(res)))
        n = res.n_reads + 1
        ov_t = C.c_uint8 if overlap_width == 1 else C.c_uint16
        out = {"next_read": np.ctypeslib.as_array(res.next_read, shape=(n,)).copy(),
               "overlap": np.ctypeslib.as_array(C.cast(res.overlap, C.POINTER(ov_t)), shape=(n,)).copy(),
               "reads_left": np.ctypeslib.as_array(res.reads_left_after, shape=(res.n_left,)).copy(),
               "duplicates": res.duplicates, "links": res.links, "sweeps": res.sweeps}
        finder.n_reads = res.n_reads
        finder.sweeps = res.sweeps
        lib.pgrc_ovl_free_result(C.byref(res))
        return out

    def to_matcher(self, matcher) -> None:
        """the LQ rows, then the N rows, become the matcher's reads (MatchContext.set_reads_packed_sets from the device)"""
        i = self.info()
        self._ck(lib.pgrc_rsets_to_matcher(self._h, matcher._h))
        matcher.n = i["count"][1] + i["count"][2]

    def timing(self) -> dict:
        t = _lib.RsetsTiming(C.sizeof(_lib.RsetsTiming))
        self._ck(lib.pgrc_rsets_get_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_ if k != "struct_size"}

    def close(self) -> None:
        if self._h:
            lib.pgrc_rsets_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
