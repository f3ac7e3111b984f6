"""include/pgrc_readslist_ord.h, the order-preserving mode of the reads list: its four names are exported by
libpgrc_rlist_ord.so, declared in the header and bound in pgrc_amd/_lib.py (RLIST_ORD_PROTOS), and libpgrc_match.so exports
none of them and gained nothing but pgrc_decode_set_order_positions; the two new structs are laid out in _lib.py as the header
lays them out (a C99 program compiled with -pedantic -Werror and linked against both libraries prints sizes and offsets and
calls the four); the sizes of the existing structs are unchanged.  No GPU: without a device pgrc_rlist_create fails, and the
text of a refusal lives in a list handle, so the wrong-struct_size refusals are asserted in tests/test_gpu_rlist_ord.py."""
import ctypes as C
import os
import re
import subprocess

from test_abi_rlist import OLD_SIZES, SIZES, exported_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_PARAM = 1
SYMBOLS = ("pgrc_rlist_export_original_order", "pgrc_rlist_archive_encode_ord", "pgrc_rlist_positions", "pgrc_rlist_positions_free")
STRUCTS = {"pgrc_rlist_export_org_args": "RlistExportOrgArgs", "pgrc_rlist_positions_out": "RlistPositionsOut"}
NEW_SIZES = {"pgrc_rlist_export_org_args": 40, "pgrc_rlist_positions_out": 40}


def names_of(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_the_four_symbols_are_exported_declared_and_bound():
    from pgrc_amd import _lib, decode
    product, own = exported_names(), names_of(_lib.RLIST_ORD_LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pgrc_readslist_ord.h")).read()
    declared = set(re.findall(r"^(?:int|void) (pgrc_rlist_\w+)\(", header, flags=re.M))
    assert declared == set(SYMBOLS) == set(_lib.RLIST_ORD_EXPORTED_SYMBOLS) and set(SYMBOLS) <= own
    assert all(getattr(_lib.olib, s).argtypes is not None for s in SYMBOLS) and _lib.olib.pgrc_rlist_positions_free.restype is None
    # the library of their own holds the product's objects and these four: nothing else is newly visible in it ...
    assert own - product == set(SYMBOLS) and product <= own
    # ... and the product library exports none of them, a list of their own mirrors them, and its one new name is the decoder's
    assert not set(SYMBOLS) & product and not set(SYMBOLS) & set(_lib.RLIST_EXPORTED_SYMBOLS)
    assert "pgrc_decode_set_order_positions" in product and "pgrc_decode_set_order_positions" in [p[0] for p in decode.DECODE_PROTOS]
    assert "pgrc_decode_set_order_positions(" in open(os.path.join(ROOT, "include", "pgrc_decode.h")).read()
    assert not [n for n in own if not n.startswith("pgrc_")]
    assert not [n for n in own if any(h in n for h in ("order_resident", "resident_release", "positions_build", "take_export", "pgrc_rl_"))]
    nm = subprocess.run(["nm", "-C", _lib.RLIST_ORD_LIB_PATH], capture_output=True, text=True).stdout
    assert "rocprim" not in nm                          # no library kernel
    import pgrc_amd
    for m in ("export_original_order", "archive_encode_ord", "positions"):
        assert callable(getattr(pgrc_amd.ReadsList, m))
    assert callable(pgrc_amd.PgRCDecoder.set_order_positions)
    assert (_lib.RLIST_CALLS[8], _lib.RLIST_CALLS[9]) == ("export_original_order", "positions")


def test_layout_of_the_new_structs_and_sizes_of_the_old(tmp_path):
    from pgrc_amd import _lib
    old = dict(OLD_SIZES, **SIZES)
    assert SIZES == {"pgrc_rlist_info": 40, "pgrc_rlist_timing": 48, "pgrc_rlist_export_args": 48, "pgrc_rlist_archive": 56 + 4168, "pgrc_rlist_pairpos_args": 80}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pgrc_readslist_ord.h"', 'int main(void) {']
    for cname, pyname in STRUCTS.items():
        lines.append(f'    printf("%zu\\n", sizeof({cname}));')
        for f, _ in getattr(_lib, pyname)._fields_:
            lines.append(f'    printf("%zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname} *)0)->{f}));')
    lines += [f'    printf("%zu\\n", sizeof({c}));' for c in old]
    lines += ['    printf("%d %d\\n", PGRC_RLIST_EXPORT_ORIGINAL, PGRC_RLIST_PAIR_POSITIONS);',
              '    pgrc_rlist_positions_free(NULL);',
              '    printf("%d %d %d\\n", pgrc_rlist_export_original_order(NULL, NULL, NULL), pgrc_rlist_archive_encode_ord(NULL, 0, NULL),',
              '           pgrc_rlist_positions(NULL, NULL));', '    return 0;', '}']
    src = tmp_path / "rlist_ord.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "rlist_ord"
    libdir = os.path.dirname(_lib.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lpgrc_rlist_ord", "-lpgrc_match", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = iter(subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n"))
    for cname, pyname in STRUCTS.items():
        st = getattr(_lib, pyname)
        assert int(next(out)) == C.sizeof(st) == NEW_SIZES[cname], cname
        assert st._fields_[0][0] == "struct_size"
        for f, _ in st._fields_:
            off, size = (int(x) for x in next(out).split())
            d = getattr(st, f)
            assert (d.offset, d.size) == (off, size), (cname, f)
    for cname, size in old.items():
        assert int(next(out)) == size, cname
    assert next(out).split() == ["8", "7"]
    assert next(out).split() == ["1", "1", "1"]          # PGRC_E_PARAM from each


def test_null_arguments_are_refused_without_a_device():
    from pgrc_amd import _lib
    lib = _lib.olib
    a = _lib.RlistExportOrgArgs(C.sizeof(_lib.RlistExportOrgArgs))
    ar = _lib.RlistArchive()
    assert lib.pgrc_rlist_export_original_order(None, None, C.byref(a)) == E_PARAM
    assert lib.pgrc_rlist_archive_encode_ord(None, 0, C.byref(ar)) == E_PARAM
    p = _lib.RlistPairPosArgs(C.sizeof(_lib.RlistPairPosArgs), 4, 0)
    o = _lib.RlistPositionsOut(C.sizeof(_lib.RlistPositionsOut))
    assert lib.pgrc_rlist_positions(None, C.byref(o)) == E_PARAM and lib.pgrc_rlist_positions(C.byref(p), C.byref(o)) == E_PARAM      # no HQ list
    lib.pgrc_rlist_positions_free(None)
    lib.pgrc_rlist_positions_free(C.byref(o))           # an empty struct: nothing to give back
    assert bytes(o) == bytes(C.sizeof(o))
    assert _lib.lib.pgrc_decode_set_order_positions(None, None, 4, 0, 0) == E_PARAM


def test_create_still_names_the_missing_device():
    import torch
    from pgrc_amd import _lib
    if torch.cuda.is_available():
        return
    h = C.c_void_p()
    assert _lib.lib.pgrc_rlist_create(-1, C.byref(h)) == 3 and not h.value
    assert _lib.lib.pgrc_rlist_last_error(None) == b"reads list: no HIP device"
