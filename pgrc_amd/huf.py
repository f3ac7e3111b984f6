"""Host-side mirror of the Huffman mode of the reference's coder type 5 (FSE_HUF_CODER with getDefaultHufCoderProps;
coders/FSECoder.{h,cpp}) over include/pgrc_huf.h, on the MI355X.  No compute here.

Sources and coded streams are host arrays (bytes, bytearray, numpy uint8), torch device tensors (uint8, contiguous) or a tuple
(device address, length); device memory is handed over by its address and never copied to the host.  A HufCoder also is the
archive container's plug-in pair: compress(src, coder=h.coder) and decompress(archive, decoder=h.decoder())."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import PgrcMatchError, hlib
from .archive import FSE_HUF_CODER
from .varlen import _is_tensor, _view, _wait_for_torch

MODE_HUF, MODE_FSE = 0, 1       # FSECoderProps::HUF_MODE / FSE_MODE (coders/FSECoder.h:19-20)


class HufCoder:
    """FSECompress / FSEUncompress in Huffman mode (coders/FSECoder.cpp:15-135) on the device"""

    def __init__(self, device: int = 0, block_order: int = 17, table_log: int = 11):
        self._h = C.c_void_p()
        self.device, self.block_order, self.table_log = int(device), int(block_order), int(table_log)
        rc = hlib.pgrc_huf_create(self.device, C.byref(self._h))
        if rc:
            raise PgrcMatchError(rc, (hlib.pgrc_huf_last_error(None) or b"").decode())

    def _ck(self, rc: int) -> None:
        if rc:
            raise PgrcMatchError(rc, (hlib.pgrc_huf_last_error(self._h) or b"").decode())

    def bound(self, n: int) -> int:
        return int(hlib.pgrc_huf_bound(int(n), self.block_order))

    def encode(self, data, out=None):
        """data: the source, or a tuple (device address, length) complete before the call.  out: a uint8 host array or
        device tensor to write into; without it, a device tensor when data is one, else a host array.  -> the payload (a
        view of out): the four props bytes and the chunks"""
        keep, sptr, n, sdev = _view(data)
        if out is None:
            cap = max(self.bound(n), 4)
            if sdev and _is_tensor(keep):
                import torch
                out = torch.empty(cap, dtype=torch.uint8, device=keep.device)
            else:
                out = np.empty(cap, dtype=np.uint8)
        elif not _is_tensor(out) and not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError("out: a writeable contiguous uint8 array or a device tensor")
        _, optr, ocap, odev = _view(out)
        got = C.c_uint64(0)
        _wait_for_torch(keep, out)
        self._ck(hlib.pgrc_huf_encode(self._h, sptr, n, sdev, self.block_order, self.table_log, optr, ocap, odev, C.byref(got)))
        return out[:got.value]

    def decode(self, payload, dest_len: int, out=None):
        """payload: a coded stream; dest_len: the decoded length.  -> the bytes, a device tensor if `payload` is one"""
        keep, cptr, clen, cdev = _view(payload)
        n = int(dest_len)
        if out is None:
            if cdev and _is_tensor(keep):
                import torch
                out = torch.empty(max(n, 1), dtype=torch.uint8, device=keep.device)
            else:
                out = np.empty(max(n, 1), dtype=np.uint8)
        _, optr, ocap, odev = _view(out)
        if ocap < n:
            raise ValueError("out is shorter than the expected length")
        _wait_for_torch(keep, out)
        self._ck(hlib.pgrc_huf_decode(self._h, cptr, clen, cdev, n, optr, odev))
        return out[:n]

    # ---- the archive container's plug-ins (pgrc_amd/archive.py)
    def coder(self, name: str, data):
        """the writer plug-in: every stream in Huffman mode; the container stores what does not shrink"""
        return FSE_HUF_CODER, self.encode(data).tobytes()

    def decoder(self, fallback=None):
        """the reader plug-in: type 5 in Huffman mode is decoded here; every other type, and type 5 in FSE mode, goes to
        `fallback` (None without one: the container then names the stream it has no decoder for)"""
        def decode(coder_type, payload, dest_len):
            if coder_type == FSE_HUF_CODER and len(payload) >= 1 and payload[0] == MODE_HUF:
                return self.decode(payload, dest_len).tobytes()
            return fallback(coder_type, payload, dest_len) if fallback is not None else None
        return decode

    def timing(self) -> dict:
        """the last encode or decode in milliseconds (introspection: tests, tools)"""
        t = _lib.HufTimes()
        self._ck(hlib.pgrc_huf_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_}

    def close(self) -> None:
        if self._h:
            hlib.pgrc_huf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
