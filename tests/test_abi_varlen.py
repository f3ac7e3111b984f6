"""The entry points of include/pgrc_varlen.h and the ones pgrc_mem.h and pgrc_decode.h gained with it: exported by the
library, declared in the Python mirror, present in the headers; pgrc_varlen_part and pgrc_varlen_times laid out in
pgrc_amd/_lib.py as the C header lays them out (sizes and offsets printed by a C program compiled against the header); NULL
arguments refused without a device; and pgrc_varlen_create, which checks the book before it looks for a device, refusing a
bad book with PGRC_E_PARAM and a good one, on a machine without a device, with PGRC_E_NO_DEVICE.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

import varlen_util as vu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_PARAM, E_NO_DEVICE = 1, 3
VARLEN = ("pgrc_varlen_create", "pgrc_varlen_destroy", "pgrc_varlen_last_error", "pgrc_varlen_bound", "pgrc_varlen_encode",
          "pgrc_varlen_decode", "pgrc_varlen_timing")
MEM = ("pgrc_mem_mark_and_remove_resident", "pgrc_mem_encode_mapped")
DECODE = ("pgrc_decode_set_mapped_text_coded",)
STRUCTS = {"pgrc_varlen_part": "VarLenPart", "pgrc_varlen_times": "VarLenTimes"}


def fixture_book() -> bytes:
    _, _, streams = vu.load_fixtures()[0]
    return vu.parse_stream(streams[0])[2].raw + b"\0"


def test_symbols_are_exported_declared_and_in_the_headers():
    from pgrc_amd import _lib, decode
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for header, symbols, declared in (("pgrc_varlen.h", VARLEN, _lib.VARLEN_EXPORTED_SYMBOLS), ("pgrc_mem.h", MEM, _lib.EXPORTED_SYMBOLS),
                                      ("pgrc_decode.h", DECODE, [p[0] for p in decode.DECODE_PROTOS])):
        text = open(os.path.join(ROOT, "include", header)).read()
        for s in symbols:
            assert s in names, f"{s} is not exported"
            assert s in declared and hasattr(_lib.lib, s) and getattr(_lib.lib, s).argtypes is not None
            assert s + "(" in text, f"{s} is not in {header}"
    assert set(_lib.VARLEN_EXPORTED_SYMBOLS) == set(VARLEN)
    assert _lib.lib.pgrc_varlen_bound.restype is C.c_uint64 and _lib.lib.pgrc_varlen_destroy.restype is None
    assert _lib.lib.pgrc_varlen_encode.argtypes[4] is C.c_uint64 and _lib.lib.pgrc_varlen_decode.argtypes[4] is C.c_uint64


def test_struct_layout_equals_the_headers(tmp_path):
    from pgrc_amd import _lib
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pgrc_varlen.h"', '#include "pgrc_mem.h"', '#include "pgrc_decode.h"',
             'int main(void) {']
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
    lib = _lib.lib
    n = C.c_uint64(7)
    lens = (C.c_uint64 * 3)()
    part = _lib.VarLenPart()
    assert lib.pgrc_varlen_create(fixture_book(), 10, 0, None) == E_PARAM
    h = C.c_void_p(1)
    assert lib.pgrc_varlen_create(None, 0, 0, C.byref(h)) == E_PARAM and not h.value
    assert lib.pgrc_varlen_encode(None, C.byref(part), 1, None, 0, 0, C.byref(n)) == E_PARAM
    assert lib.pgrc_varlen_decode(None, None, 0, 0, 0, None, 0) == E_PARAM
    assert lib.pgrc_varlen_timing(None, None) == E_PARAM
    lib.pgrc_varlen_destroy(None)
    assert lib.pgrc_varlen_bound(0) == 0 and lib.pgrc_varlen_bound((1 << 32) + 4099) == (1 << 32) + 4099
    mp = _lib.MemMapping()
    assert lib.pgrc_mem_mark_and_remove_resident(None, None, 0, 40, 0, C.byref(mp)) == E_PARAM
    assert lib.pgrc_mem_encode_mapped(None, None, None, 0, C.byref(n), C.byref(lens)) == E_PARAM
    assert lib.pgrc_decode_set_mapped_text_coded(None, None, None, None, 0) == E_PARAM


@pytest.mark.parametrize("what,book", [
    ("257 codes", b"\n".join([b"A", b"C", b"G", b"T"] + [b""] * 253)),
    ("a 5-byte code", b"A\nC\nG\nT\nACGTA"),
    ("a two-symbol code 0", b"AC\nA\nC"),
    ("a symbol without a one-symbol code", b"A\nC\nAG"),
    ("two symbols sharing their low three bits", b"A\nC\nG\nT\nI"),       # 'A' 0x41, 'I' 0x49
    ("a symbol whose low three bits are 0", b"A\nC\nG\nT\nH"),            # 'H' 0x48
])
def test_create_checks_the_book_before_the_device(what, book):
    from pgrc_amd import _lib
    h = C.c_void_p()
    assert _lib.lib.pgrc_varlen_create(book, len(book), 0, C.byref(h)) == E_PARAM, what
    assert not h.value and _lib.lib.pgrc_varlen_last_error(None)


def test_create_without_a_device_is_no_device():
    import torch
    from pgrc_amd import PgrcMatchError, VarLenDNACoder
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the GPU tests cover everything past the creation")
    with pytest.raises(PgrcMatchError) as e:
        VarLenDNACoder(fixture_book())
    assert e.value.code == E_NO_DEVICE
