"""include/pgrc_readsets.h: the exported pgrc_rsets_* names are the header's and the Python mirror's, the structs are laid
out in pgrc_amd/_lib.py as the header lays them out (compiled from C99 with -pedantic -Werror), NULL arguments are refused
without a device, and the structs the other headers had before keep their sizes.  No GPU: without a device pgrc_rsets_create
fails, so of the refusals only the ones in front of it are asserted here (tests/test_gpu_rsets.py has the rest)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"pgrc_rsets_params": "RsetsParams", "pgrc_rsets_info": "RsetsInfo", "pgrc_rsets_timing": "RsetsTiming"}
SIZES = {"pgrc_rsets_params": 20, "pgrc_rsets_info": 80, "pgrc_rsets_timing": 40}
OLD_SIZES = {"pgrc_ovl_input": 48, "pgrc_ovl_result": 64, "pgrc_divided_reads": 88, "pgrc_divide_params": 32}


def test_symbols_are_exported_and_declared():
    from pgrc_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "pgrc_readsets.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*) ?(pgrc_rsets_\w+)\(", header, flags=re.M))
    exported = {n for n in names if n.startswith("pgrc_rsets_")}
    assert exported == declared == set(_lib.RSETS_EXPORTED_SYMBOLS) and len(exported) == 17
    assert all(hasattr(_lib.lib, s) for s in exported)
    assert not set(_lib.RSETS_EXPORTED_SYMBOLS) & set(_lib.EXPORTED_SYMBOLS)            # a list of its own, never in _PROTOS
    assert _lib.RSETS_WHICH == {"hq": 0, "lq": 1, "n": 2}
    # what the other .hip files reach of one another stays hidden
    assert not [n for n in names if "last_device" in n or "append_rows_device" in n or n.startswith("pgovl_")]
    import pgrc_amd
    assert pgrc_amd.DividedReadsSets.__module__ == "pgrc_amd.readsets"


def test_layout_from_c(tmp_path):
    from pgrc_amd import _lib
    src = tmp_path / "rsets.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pgrc_readsets.h"', 'int main(void) {']
    for cname, pyname in STRUCTS.items():
        lines.append(f'    printf("%zu\\n", sizeof({cname}));')
        for f, _ in getattr(_lib, pyname)._fields_:
            lines.append(f'    printf("%zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname} *)0)->{f}));')
    lines += [f'    printf("%zu\\n", sizeof({c}));' for c in OLD_SIZES]
    lines += ['    printf("%d %d %d %d\\n", pgrc_rsets_create(NULL, NULL), pgrc_rsets_finish(NULL), pgrc_rsets_move_lq(NULL, NULL, 0),',
              '           PGRC_RSETS_HQ + 2 * PGRC_RSETS_LQ + 4 * PGRC_RSETS_N);',
              '    return 0;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "rsets"
    libdir = os.path.dirname(_lib.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lpgrc_match", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = iter(subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n"))
    for cname, pyname in STRUCTS.items():
        st = getattr(_lib, pyname)
        assert int(next(out)) == C.sizeof(st) == SIZES[cname], cname
        for f, _ in st._fields_:
            off, size = (int(x) for x in next(out).split())
            d = getattr(st, f)
            assert (d.offset, d.size) == (off, size), (cname, f)
    for cname, size in OLD_SIZES.items():
        assert int(next(out)) == size, cname
    assert next(out).split() == ["1", "1", "1", "10"]


def test_null_arguments_are_refused_without_a_device():
    from pgrc_amd import _lib
    lib = _lib.lib
    h = C.c_void_p()
    assert lib.pgrc_rsets_create(None, None) == 1 and lib.pgrc_rsets_create(None, C.byref(h)) == 1 and not h.value
    prm = _lib.RsetsParams(C.sizeof(_lib.RsetsParams) - 4, 100, 1, 0, -1)
    assert lib.pgrc_rsets_create(C.byref(prm), C.byref(h)) == 1 and b"struct_size" in lib.pgrc_rsets_last_error(None)
    for read_len in (0, 256):
        prm = _lib.RsetsParams(C.sizeof(_lib.RsetsParams), read_len, 1, 0, -1)
        assert lib.pgrc_rsets_create(C.byref(prm), C.byref(h)) == 1 and b"read length" in lib.pgrc_rsets_last_error(None)
    lib.pgrc_rsets_destroy(None)
    assert lib.pgrc_rsets_append(None, None, 0) == 1 and lib.pgrc_rsets_append_divider(None, None) == 1 and lib.pgrc_rsets_finish(None) == 1
    assert lib.pgrc_rsets_get_info(None, None) == 1 and lib.pgrc_rsets_get_rows(None, 0, 0, 0, None) == 1
    assert lib.pgrc_rsets_get_mapping(None, 0, None) == 1 and lib.pgrc_rsets_dispose(None, 0) == 1
    assert lib.pgrc_rsets_move_lq(None, None, 0) == 1 and lib.pgrc_rsets_move_by_overlap(None, None) == 1
    assert lib.pgrc_rsets_remove(None, None, 0) == 1 and lib.pgrc_rsets_remove_matched(None, None) == 1
    assert lib.pgrc_rsets_overlap(None, 0, None, 1.0, 1, None, None) == 1 and lib.pgrc_rsets_to_matcher(None, None) == 1
    assert lib.pgrc_rsets_get_timing(None, None) == 1
    assert C.sizeof(_lib.OvlInput) == 48 and C.sizeof(_lib.OvlResult) == 64
    assert C.sizeof(_lib.DividedReads) == 88 and C.sizeof(_lib.DivideParams) == 32
