"""The device-text entry points of include/pgrc_mem.h (pgrc_mem_set_src_device, pgrc_mem_match_texts_device): exported by the
library, declared in the header and in the Python mirror with the host forms' argument lists, and refusing a NULL context.  No
GPU: without a device pgrc_mem_create fails as it always did, so nothing past it is asserted here."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pgrc_mem_set_src_device", "pgrc_mem_match_texts_device")
E_PARAM, E_NO_DEVICE = 1, 3


def test_symbols_are_exported_and_declared():
    from pgrc_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "pgrc_mem.h")).read()
    for s in SYMBOLS:
        assert s in names, f"{s} is not exported"
        assert hasattr(_lib.lib, s)
        assert s + "(" in header
    # the device forms take what the host forms take, a device address in place of the host pointer
    assert _lib.lib.pgrc_mem_set_src_device.argtypes == _lib.lib.pgrc_mem_set_src_ascii.argtypes
    assert _lib.lib.pgrc_mem_match_texts_device.argtypes == _lib.lib.pgrc_mem_match_texts.argtypes
    assert _lib.lib.pgrc_mem_set_src_device.restype is C.c_int and _lib.lib.pgrc_mem_match_texts_device.restype is C.c_int


def test_the_python_mirror_has_the_device_forms():
    from pgrc_amd import CopMEMMatcher
    assert callable(CopMEMMatcher.setSrcDevice) and callable(CopMEMMatcher.matchTextsDevice)


def test_a_null_context_is_refused_without_a_device():
    from pgrc_amd import _lib
    lib = _lib.lib
    out, cnt = C.POINTER(_lib.TextMatch)(), C.c_uint64(7)
    assert lib.pgrc_mem_set_src_device(None, None, 0) == E_PARAM
    assert lib.pgrc_mem_set_src_device(None, C.c_void_p(4096), 100) == E_PARAM
    assert lib.pgrc_mem_match_texts_device(None, None, 0, 1, 1, 45, C.byref(out), C.byref(cnt)) == E_PARAM
    assert lib.pgrc_mem_match_texts_device(None, C.c_void_p(4096), 100, 0, 1, 45, C.byref(out), C.byref(cnt)) == E_PARAM
    assert not out and cnt.value == 7                       # (nothing was written)


def test_create_fails_without_a_device():
    import torch
    from pgrc_amd import CopMEMMatcher, PgrcMatchError
    if torch.cuda.is_available():
        return                                              # (with a device the GPU tests cover everything past the creation)
    with pytest.raises(PgrcMatchError) as e:
        CopMEMMatcher(None, 45)                             # the form without a host text
    assert e.value.code == E_NO_DEVICE
