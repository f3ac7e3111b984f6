"""The mapping entry points of include/pgrc_mem.h (pgrc_mem_mark_and_remove, pgrc_mem_free_mapping and the phase timing):
exported by the library, declared in the Python mirror, and pgrc_mem_mapping laid out in pgrc_amd/_lib.py as the C header
lays it out (sizes and offsets printed by a C program compiled against the header).  No GPU: without a device
pgrc_mem_create fails as it always did, so nothing past it is asserted here."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pgrc_mem_mark_and_remove", "pgrc_mem_free_mapping", "pgrc_mem_mapping_timing")
FIELDS = ("mapped_len", "marks", "unique_matches", "matched_symbols", "map_off", "map_off_bytes", "map_len", "map_len_bytes")


def test_symbols_are_exported_and_declared():
    from pgrc_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "pgrc_mem.h")).read()
    for s in SYMBOLS:
        assert s in names, f"{s} is not exported"
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, s)
        assert s + "(" in header
    assert _lib.lib.pgrc_mem_mark_and_remove.argtypes[2:4] == [C.c_uint64, C.c_uint32]
    assert _lib.lib.pgrc_mem_free_mapping.restype is None


def test_struct_layout_equals_the_headers(tmp_path):
    from pgrc_amd import _lib
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pgrc_mem.h"', 'int main(void) {',
             '    printf("%zu\\n", sizeof(pgrc_mem_mapping));']
    lines += [f'    printf("%zu %zu\\n", offsetof(pgrc_mem_mapping, {f}), sizeof(((pgrc_mem_mapping *)0)->{f}));' for f in FIELDS]
    lines += ['    printf("%zu\\n", sizeof(pgrc_text_match));', '    return 0;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == C.sizeof(_lib.MemMapping)
    assert [f for f, _ in _lib.MemMapping._fields_] == list(FIELDS)
    for f, ln in zip(FIELDS, out[1:]):
        off, size = (int(x) for x in ln.split())
        d = getattr(_lib.MemMapping, f)
        assert (d.offset, d.size) == (off, size), f
    assert int(out[1 + len(FIELDS)]) == C.sizeof(_lib.TextMatch)


def test_null_arguments_are_refused_without_a_device():
    from pgrc_amd import _lib
    mp = _lib.MemMapping()
    assert _lib.lib.pgrc_mem_mark_and_remove(None, None, 0, 40, None, 0, C.byref(mp)) == 1       # PGRC_E_PARAM
    _lib.lib.pgrc_mem_free_mapping(C.byref(mp))                                                  # (an empty one: nothing to free)
    _lib.lib.pgrc_mem_free_mapping(None)
    assert _lib.lib.pgrc_mem_mapping_timing(None, None) == 1


def test_create_still_fails_without_a_device():
    import torch
    from pgrc_amd import CopMEMMatcher, PgrcMatchError
    if torch.cuda.is_available():
        return                                              # (with a device the GPU tests cover everything past the creation)
    with pytest.raises(PgrcMatchError) as e:
        CopMEMMatcher(b"ACGT" * 100, 40)
    assert e.value.code == 3
