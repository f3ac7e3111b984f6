"""The entry points of include/pgrc_overlap.h: exported by the library, declared in the Python mirror, and pgrc_ovl_input,
pgrc_ovl_result and pgrc_ovl_timing laid out in pgrc_amd/_lib.py as the C header lays them out (sizes and offsets printed
by a C99 program compiled against the header).  No GPU: without a device pgrc_ovl_create fails, so nothing past it is
asserted here."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pgrc_ovl_create", "pgrc_ovl_destroy", "pgrc_ovl_last_error", "pgrc_ovl_run", "pgrc_ovl_free_result", "pgrc_ovl_both_sides",
           "pgrc_ovl_assemble", "pgrc_ovl_get_timing", "pgrc_ovl_get_sweep_ms")
STRUCTS = {
    "pgrc_ovl_input": ("OvlInput", ("struct_size", "read_len", "symbols", "overlap_width", "n_reads", "stop_coef", "packed_rows", "sorted_order")),
    "pgrc_ovl_result": ("OvlResult", ("struct_size", "sweeps", "n_reads", "n_left", "duplicates", "links", "next_read", "overlap", "reads_left_after")),
    "pgrc_ovl_timing": ("OvlTiming", ("struct_size", "passes", "ms_upload", "ms_order_device", "ms_start_device", "ms_merge_device", "ms_pair_device",
                                      "ms_compact_device", "ms_download", "ms_call", "bytes_up", "bytes_down")),
}


def test_symbols_are_exported_and_declared():
    from pgrc_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "pgrc_overlap.h")).read()
    for s in SYMBOLS:
        assert s in names, f"{s} is not exported"
        assert s in _lib.OVL_EXPORTED_SYMBOLS and hasattr(_lib.lib, s)
        assert s + "(" in header
    assert {n for n in names if n.startswith("pgrc_ovl_")} == set(SYMBOLS) == set(_lib.OVL_EXPORTED_SYMBOLS)
    assert _lib.lib.pgrc_ovl_free_result.restype is None and _lib.lib.pgrc_ovl_destroy.restype is None
    import pgrc_amd
    assert pgrc_amd.OverlapFinder is pgrc_amd.overlap.OverlapFinder


def test_struct_layouts_equal_the_headers(tmp_path):
    from pgrc_amd import _lib
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pgrc_overlap.h"', 'int main(void) {']
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
    assert lib.pgrc_ovl_create(-1, None) == 1                   # PGRC_E_PARAM
    res = _lib.OvlResult()
    inp = _lib.OvlInput(C.sizeof(_lib.OvlInput), 40, 4, 1, 1, 1.0, None, None)
    assert lib.pgrc_ovl_run(None, C.byref(inp), C.byref(res)) == 1
    lib.pgrc_ovl_free_result(C.byref(res))                      # (an empty one: nothing to free)
    lib.pgrc_ovl_free_result(None)
    lib.pgrc_ovl_destroy(None)
    assert lib.pgrc_ovl_both_sides(None, None) == 1
    assert lib.pgrc_ovl_assemble(None, None, None, None) == 1
    assert lib.pgrc_ovl_get_timing(None, None) == 1
    assert lib.pgrc_ovl_get_sweep_ms(None, None, 0) == 1


def test_create_fails_without_a_device():
    import torch
    from pgrc_amd import OverlapFinder, PgrcMatchError
    if torch.cuda.is_available():
        return                                              # (with a device the GPU tests cover everything past the creation)
    with pytest.raises(PgrcMatchError) as e:
        OverlapFinder()
    assert e.value.code == 3                                # PGRC_E_NO_DEVICE


def test_stage_creates_name_the_missing_device():
    """the overlap search and the read sets open a stage handle of their own: without a device both creates are
    PGRC_E_NO_DEVICE, each with its own text"""
    import torch
    from pgrc_amd import _lib
    if torch.cuda.is_available():
        return
    lib = _lib.lib
    h = C.c_void_p()
    assert lib.pgrc_ovl_create(-1, C.byref(h)) == 3 and not h.value
    assert lib.pgrc_ovl_last_error(None) == b"no HIP device"
    prm = _lib.RsetsParams(C.sizeof(_lib.RsetsParams), 100, 0, 0, -1)
    assert lib.pgrc_rsets_create(C.byref(prm), C.byref(h)) == 3 and not h.value
    assert lib.pgrc_rsets_last_error(None) == b"read sets: no HIP device"
