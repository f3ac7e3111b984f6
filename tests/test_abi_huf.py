"""The entry points of include/pgrc_huf.h: exported by libpgrc_huf.so (and by it alone), declared in the Python mirror,
present in the header; pgrc_huf_times laid out in pgrc_amd/_lib.py as the C header lays it out (sizes and offsets printed by a
C program compiled against the header); NULL arguments refused without a device, and a block order outside 1 .. 17 by
pgrc_huf_bound; and HufCoder(), which on a machine without a device fails with PGRC_E_NO_DEVICE.  A handle exists only with a
device, so the range checks of pgrc_huf_encode (block order, table log) are tests/test_gpu_huf.py's.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_PARAM, E_NO_DEVICE = 1, 3
HUF = ("pgrc_huf_create", "pgrc_huf_destroy", "pgrc_huf_last_error", "pgrc_huf_bound", "pgrc_huf_encode", "pgrc_huf_decode",
       "pgrc_huf_timing")
STRUCTS = {"pgrc_huf_times": "HufTimes"}


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_symbols_are_exported_declared_and_in_the_header():
    from pgrc_amd import _lib
    names = exported(_lib.HUF_LIB_PATH)
    text = open(os.path.join(ROOT, "include", "pgrc_huf.h")).read()
    for s in HUF:
        assert s in names, f"{s} is not exported"
        assert s in _lib.HUF_EXPORTED_SYMBOLS and getattr(_lib.hlib, s).argtypes is not None
        assert s + "(" in text, f"{s} is not in pgrc_huf.h"
    assert set(_lib.HUF_EXPORTED_SYMBOLS) == set(HUF)
    assert all(n.startswith("pgrc_") for n in names), "only pgrc_* is visible"
    assert not any(n.startswith("pgrc_huf") for n in exported(_lib.LIB_PATH)), "libpgrc_match.so exports what it always did"
    assert _lib.hlib.pgrc_huf_bound.restype is C.c_uint64 and _lib.hlib.pgrc_huf_destroy.restype is None
    assert _lib.hlib.pgrc_huf_encode.argtypes[2] is C.c_uint64 and _lib.hlib.pgrc_huf_decode.argtypes[4] is C.c_uint64


def test_struct_layout_equals_the_header(tmp_path):
    from pgrc_amd import _lib
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pgrc_huf.h"', 'int main(void) {']
    for cname, pyname in STRUCTS.items():
        lines.append(f'    printf("%zu\\n", sizeof({cname}));')
        for f, _ in getattr(_lib, pyname)._fields_:
            lines.append(f'    printf("%zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname} *)0)->{f}));')
    lines += ['    return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = iter(subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n"))
    for cname, pyname in STRUCTS.items():
        st = getattr(_lib, pyname)
        assert int(next(out)) == C.sizeof(st), cname
        for f, _ in st._fields_:
            off, size = (int(x) for x in next(out).split())
            d = getattr(st, f)
            assert (d.offset, d.size) == (off, size), (cname, f)


def test_null_arguments_are_refused_without_a_device():
    from pgrc_amd import _lib
    lib = _lib.hlib
    n = C.c_uint64(7)
    buf = C.create_string_buffer(64)
    assert lib.pgrc_huf_create(0, None) == E_PARAM
    assert lib.pgrc_huf_encode(None, buf, 8, 0, 17, 11, buf, 64, 0, C.byref(n)) == E_PARAM
    assert lib.pgrc_huf_decode(None, buf, 8, 0, 4, buf, 0) == E_PARAM
    assert lib.pgrc_huf_timing(None, None) == E_PARAM
    lib.pgrc_huf_destroy(None)
    assert lib.pgrc_huf_last_error(None) is not None


def test_bound_is_the_raw_frame_and_refuses_a_bad_order():
    from pgrc_amd import _lib
    b = _lib.hlib.pgrc_huf_bound
    assert b(0, 17) == 4 and b(1, 17) == 5 and b(1 << 17, 17) == 4 + (1 << 17) and b((1 << 17) + 1, 17) == 4 + (1 << 17) + 1 + 4
    assert b(2049, 10) == 4 + 2049 + 8 and b((1 << 32) + 5, 17) == 4 + (1 << 32) + 5 + 4 * (1 << 15)
    assert b(100, 0) == 0 and b(100, 18) == 0


def test_the_python_mirror_states_the_headers_limits():
    from pgrc_amd import _lib
    text = open(os.path.join(ROOT, "include", "pgrc_huf.h")).read()
    for name, value in (("PGRC_HUF_ORDER_MAX", _lib.HUF_ORDER_MAX), ("PGRC_HUF_TABLE_LOG_MIN", _lib.HUF_TABLE_LOG_MIN),
                        ("PGRC_HUF_TABLE_LOG_MAX", _lib.HUF_TABLE_LOG_MAX)):
        assert f"#define {name} {value}\n" in text


def test_create_without_a_device_is_no_device():
    import torch
    from pgrc_amd import HufCoder, PgrcMatchError
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the GPU tests cover everything past the creation")
    with pytest.raises(PgrcMatchError) as e:
        HufCoder()
    assert e.value.code == E_NO_DEVICE
