"""The entry points of the archive form of a list's mismatch streams (include/pgrc_decode.h, "The archive form"): exported by
the library, declared in the Python mirror, present in the header; pgrc_list_archive_streams and pgrc_list_archive_timing laid
out in pgrc_amd/_lib.py as the C header lays them out (sizes and offsets printed by a C program compiled against the header);
NULL arguments refused without a device; and a decode context, which every call works on, is PGRC_E_NO_DEVICE without one.
No GPU."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_PARAM, E_NO_DEVICE = 1, 3
SYMBOLS = ("pgrc_list_archive_encode", "pgrc_list_archive_free", "pgrc_decode_add_list_archive", "pgrc_list_archive_get_timing")
STRUCTS = {"pgrc_list_archive_streams": "ListArchiveStreams", "pgrc_list_archive_timing": "ListArchiveTiming"}


def test_symbols_are_exported_declared_and_in_the_header():
    from pgrc_amd import _lib, decode
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    text = open(os.path.join(ROOT, "include", "pgrc_decode.h")).read()
    declared = [p[0] for p in decode.DECODE_PROTOS]
    for s in SYMBOLS:
        assert s in names, f"{s} is not exported"
        assert s in declared and hasattr(_lib.lib, s) and getattr(_lib.lib, s).argtypes is not None
        assert s + "(" in text, f"{s} is not in pgrc_decode.h"
    assert _lib.lib.pgrc_list_archive_free.restype is None
    assert f"#define PGRC_LIST_ARCHIVE_TILE {decode.PGRC_LIST_ARCHIVE_TILE}u" in text
    nm = subprocess.run(["nm", "-C", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "rocprim" not in nm                          # no library kernel


def test_struct_layout_equals_the_header(tmp_path):
    from pgrc_amd import _lib
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pgrc_decode.h"', 'int main(void) {']
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
    from pgrc_amd.decode import DecodeList
    lib = _lib.lib
    x, s, t, a = _lib.ExportStreams(), _lib.ListArchiveStreams(), _lib.ListArchiveTiming(), DecodeList()
    assert lib.pgrc_list_archive_encode(None, C.byref(x), 0, C.byref(s)) == E_PARAM
    assert lib.pgrc_list_archive_encode(None, None, 0, None) == E_PARAM
    assert lib.pgrc_decode_add_list_archive(None, C.byref(a), C.byref(s)) == E_PARAM
    assert lib.pgrc_decode_add_list_archive(None, None, None) == E_PARAM
    assert lib.pgrc_list_archive_get_timing(None, C.byref(t)) == E_PARAM
    assert lib.pgrc_list_archive_get_timing(None, None) == E_PARAM
    lib.pgrc_list_archive_free(None)
    lib.pgrc_list_archive_free(C.byref(s))              # an empty struct: nothing to give back
    assert bytes(s) == bytes(C.sizeof(s))


def test_without_a_device_is_no_device():
    import torch
    from pgrc_amd import PgRCDecoder, PgrcMatchError
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the GPU tests cover everything past the creation")
    with pytest.raises(PgrcMatchError) as e:
        PgRCDecoder(150)                                # the device handle of every list-archive call
    assert e.value.code == E_NO_DEVICE
