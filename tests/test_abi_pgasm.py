"""The entry points of include/pgrc_assemble.h: exported by the library, declared in the Python mirror, and pgrc_asm_input,
pgrc_asm_result and pgrc_asm_timing laid out in pgrc_amd/_lib.py as the C header lays them out (sizes and offsets printed
by a C99 program compiled against the header).  No GPU: without a device pgrc_asm_create fails, so nothing past it is
asserted here."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pgrc_asm_create", "pgrc_asm_destroy", "pgrc_asm_last_error", "pgrc_asm_run", "pgrc_asm_free_result", "pgrc_asm_get_text",
           "pgrc_asm_text_device", "pgrc_asm_packed_device", "pgrc_asm_get_timing")
STRUCTS = {
    "pgrc_asm_input": ("AsmInput", ("struct_size", "read_len", "symbols", "overlap_width", "n_reads", "packed_rows", "next_read", "overlap",
                                    "index_mapping")),
    "pgrc_asm_result": ("AsmResult", ("struct_size", "reserved", "pg_len", "n_reads", "cycles", "overlap_lost", "components", "singles",
                                      "org_idx", "off")),
    "pgrc_asm_timing": ("AsmTiming", ("struct_size", "passes_cycles", "passes_rank", "ms_upload", "ms_checks_device", "ms_cycles_device",
                                      "ms_rank_device", "ms_lists_device", "ms_text_device", "ms_download", "ms_call", "bytes_up",
                                      "bytes_down")),
}


def test_symbols_are_exported_and_declared():
    from pgrc_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "pgrc_assemble.h")).read()
    for s in SYMBOLS:
        assert s in names, f"{s} is not exported"
        assert s in _lib.ASM_EXPORTED_SYMBOLS and hasattr(_lib.lib, s)
        assert s + "(" in header
    assert {n for n in names if n.startswith("pgrc_asm_")} == set(SYMBOLS) == set(_lib.ASM_EXPORTED_SYMBOLS)
    assert _lib.lib.pgrc_asm_get_text.argtypes[1:3] == [C.c_uint64, C.c_uint64]
    assert _lib.lib.pgrc_asm_free_result.restype is None and _lib.lib.pgrc_asm_destroy.restype is None


def test_no_library_kernel_came_in():
    from pgrc_amd import _lib
    out = subprocess.run(["nm", "-C", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert sum("rocprim" in ln for ln in out.splitlines()) == 0


def test_struct_layouts_equal_the_headers(tmp_path):
    from pgrc_amd import _lib
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pgrc_assemble.h"', 'int main(void) {']
    for cname, (_, fields) in STRUCTS.items():
        lines.append(f'    printf("%zu\\n", sizeof({cname}));')
        lines += [f'    printf("%zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname} *)0)->{f}));' for f in fields]
    lines += ['    return 0;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = iter(subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n"))
    for cname, (pyname, fields) in STRUCTS.items():
        st = getattr(_lib, pyname)
        assert int(next(out)) == C.sizeof(st), cname
        assert [f for f, _ in st._fields_] == list(fields), cname
        for f in fields:
            off, size = (int(x) for x in next(out).split())
            d = getattr(st, f)
            assert (d.offset, d.size) == (off, size), (cname, f)


def test_null_arguments_are_refused_without_a_device():
    from pgrc_amd import _lib
    lib = _lib.lib
    assert lib.pgrc_asm_create(-1, None) == 1                   # PGRC_E_PARAM
    res = _lib.AsmResult()
    inp = _lib.AsmInput(C.sizeof(_lib.AsmInput), 40, 4, 1, 1, None, None, None, None)
    assert lib.pgrc_asm_run(None, C.byref(inp), C.byref(res)) == 1
    lib.pgrc_asm_free_result(C.byref(res))                      # (an empty one: nothing to free)
    lib.pgrc_asm_free_result(None)
    lib.pgrc_asm_destroy(None)
    assert lib.pgrc_asm_get_text(None, 0, 0, None) == 1
    assert lib.pgrc_asm_text_device(None, None, None) == 1
    assert lib.pgrc_asm_packed_device(None, None) == 1
    assert lib.pgrc_asm_get_timing(None, None) == 1


def test_create_fails_without_a_device():
    import torch
    from pgrc_amd import PgAssembler, PgrcMatchError
    if torch.cuda.is_available():
        return                                              # (with a device the GPU tests cover everything past the creation)
    with pytest.raises(PgrcMatchError) as e:
        PgAssembler()
    assert e.value.code == 3                                # PGRC_E_NO_DEVICE
