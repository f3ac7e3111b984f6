"""Host-side mirror of the reference's VarLenDNACoder (coders/VarLenDNACoder.h) over include/pgrc_varlen.h: the static book
of up to 256 codes of 0-4 symbols that the joined mapped pseudogenomes pass through, on the MI355X.  No compute here.

The book is an input, in the form VarLenDNACoder::writeBook gives it (it stands behind the two header bytes of a coded
stream).  Texts and coded streams are host arrays (bytes, bytearray, numpy uint8) or torch device tensors (uint8,
contiguous), which are handed over by data_ptr() and never copied to the host."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import PgrcMatchError, lib


def _is_tensor(a) -> bool:
    return hasattr(a, "data_ptr") and hasattr(a, "is_cuda")


def _wait_for_torch(*args) -> None:
    """what torch has queued on its current stream for the device tensors among args has happened"""
    for a in args:
        if _is_tensor(a) and a.is_cuda:
            import torch
            torch.cuda.current_stream(a.device).synchronize()


def _view(a):
    """-> (keep-alive object, pointer or None, length, on_device); a tuple (address, length) is raw memory of the coder's device"""
    if isinstance(a, tuple):
        ptr, n = int(a[0] or 0), int(a[1])
        return a, (ptr if n else None), n, 1
    if _is_tensor(a):
        import torch
        if a.dtype != torch.uint8 or not a.is_contiguous():
            raise ValueError("a contiguous uint8 tensor")
        return a, (a.data_ptr() if a.numel() else None), int(a.numel()), int(bool(a.is_cuda))
    if isinstance(a, str):
        a = a.encode("latin-1")
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(a, dtype=np.uint8)
    a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    return a, (a.ctypes.data if a.size else None), int(a.size), 0


class VarLenDNACoder:
    """VarLenDNACoder(codes) (VarLenDNACoder.cpp:6-35) with encode (:55-104) and decode (:106-120) on the device."""

    def __init__(self, book, device: int = -1):
        self._h = C.c_void_p()
        b = bytes(book)
        rc = lib.pgrc_varlen_create(b, len(b), int(device), C.byref(self._h))
        if rc:
            raise PgrcMatchError(rc, (lib.pgrc_varlen_last_error(None) or b"").decode())
        self.device = int(device)

    def _ck(self, rc: int) -> None:
        if rc:
            raise PgrcMatchError(rc, (lib.pgrc_varlen_last_error(self._h) or b"").decode())

    @staticmethod
    def bound(n: int) -> int:
        return int(lib.pgrc_varlen_bound(int(n)))

    def encode(self, parts, out=None):
        """parts: one text or a list of up to three (HQ | LQ | N), coded as ONE text; a part may be a tuple (device address,
        length), such as PgAssembler.text_device() gives, complete before the call (include/pgrc_varlen.h).  out: a uint8 host array or device
        tensor to write into; without it, a device tensor when every part is one, else a host array.  -> the coded
        bytes (a view of out)."""
        if _is_tensor(parts) or not isinstance(parts, (list, tuple)):
            parts = [parts]
        views = [_view(p) for p in parts]
        arr = (_lib.VarLenPart * max(len(views), 1))()
        for k, (_, ptr, n, dev) in enumerate(views):
            arr[k].ptr, arr[k].len, arr[k].on_device = ptr, n, dev
        total = sum(v[2] for v in views)
        if out is None:
            if views and all(v[3] and _is_tensor(v[0]) for v in views):
                import torch
                out = torch.empty(max(self.bound(total), 1), dtype=torch.uint8, device=views[0][0].device)
            else:
                out = np.empty(max(self.bound(total), 1), dtype=np.uint8)
        elif not _is_tensor(out) and not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError("out: a writeable contiguous uint8 array or a device tensor")
        _, optr, ocap, odev = _view(out)
        n = C.c_uint64(0)
        _wait_for_torch(out, *[v[0] for v in views])
        self._ck(lib.pgrc_varlen_encode(self._h, arr, len(views), optr, ocap, odev, C.byref(n)))
        return out[:n.value]

    def decode(self, coded, n: int, out=None):
        """coded: the payload; n: the expected decoded length.  -> the text, a device tensor if `coded` is one."""
        keep, cptr, clen, cdev = _view(coded)
        n = int(n)
        if out is None:
            if cdev:
                import torch
                out = torch.empty(max(n, 1), dtype=torch.uint8, device=keep.device)
            else:
                out = np.empty(max(n, 1), dtype=np.uint8)
        _, optr, ocap, odev = _view(out)
        if ocap < n:
            raise ValueError("out is shorter than the expected length")
        _wait_for_torch(keep, out)
        self._ck(lib.pgrc_varlen_decode(self._h, cptr, clen, cdev, n, optr, odev))
        return out[:n]

    def timing(self) -> dict:
        """the last encode or decode in milliseconds (introspection: tests, tools)"""
        t = _lib.VarLenTimes()
        self._ck(lib.pgrc_varlen_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_}

    def close(self) -> None:
        if self._h:
            lib.pgrc_varlen_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
