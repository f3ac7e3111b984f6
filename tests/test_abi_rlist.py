"""include/pgrc_readslist.h: the exported pgrc_rlist_* names are the header's and the Python mirror's; no other prefix of the
library gained a name (the hooks into the other contexts are internal C++ functions); the structs are laid out in
pgrc_amd/_lib.py as the header lays them out (a C99 program compiled with -pedantic -Werror prints sizes and offsets); NULL
arguments are refused without a device; no library kernel is linked.  No GPU: without a device pgrc_rlist_create fails, so of
the refusals only the ones in front of it are asserted here (tests/test_gpu_rlist.py has the rest)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_PARAM = 1
STRUCTS = {"pgrc_rlist_info": "RlistInfo", "pgrc_rlist_timing": "RlistTiming", "pgrc_rlist_export_args": "RlistExportArgs",
           "pgrc_rlist_archive": "RlistArchive", "pgrc_rlist_pairpos_args": "RlistPairPosArgs"}
SIZES = {"pgrc_rlist_info": 40, "pgrc_rlist_timing": 48, "pgrc_rlist_export_args": 48, "pgrc_rlist_archive": 56 + 4168, "pgrc_rlist_pairpos_args": 80}
OLD_SIZES = {"pgrc_export_streams": 80, "pgrc_list_archive_streams": 4168, "pgrc_pairorder_streams": 120, "pgrc_pairpos_streams": 112,
             "pgrc_asm_result": 72, "pgrc_rsets_info": 80}


def exported_names():
    from pgrc_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_symbols_are_exported_and_declared():
    from pgrc_amd import _lib
    names = exported_names()
    header = open(os.path.join(ROOT, "include", "pgrc_readslist.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*) ?(pgrc_rlist_\w+)\(", header, flags=re.M))
    exported = {n for n in names if n.startswith("pgrc_rlist_")}
    assert exported == declared == set(_lib.RLIST_EXPORTED_SYMBOLS) and len(exported) == 14
    assert all(hasattr(_lib.lib, s) for s in exported)
    assert not set(_lib.RLIST_EXPORTED_SYMBOLS) & set(_lib.EXPORTED_SYMBOLS)            # a list of its own, never in _PROTOS
    import pgrc_amd
    assert pgrc_amd.ReadsList.__module__ == "pgrc_amd.rlist"
    for m in ("from_assembly", "from_overlap", "export_pg_order", "download", "archive_encode", "pair_order", "pair_positions", "timing", "close"):
        assert callable(getattr(pgrc_amd.ReadsList, m))


def test_no_other_prefix_gained_a_name():
    """the counts and sets the other ABI tests pin, asserted once more beside the new names"""
    from pgrc_amd import _lib, decode
    names = exported_names()
    assert not [n for n in names if not n.startswith("pgrc_")]
    by_prefix = {"pgrc_asm_": _lib.ASM_EXPORTED_SYMBOLS, "pgrc_ovl_": _lib.OVL_EXPORTED_SYMBOLS, "pgrc_ovlrule_": _lib.OVL_RULE_EXPORTED_SYMBOLS,
                 "pgrc_rsets_": _lib.RSETS_EXPORTED_SYMBOLS, "pgrc_varlen_": _lib.VARLEN_EXPORTED_SYMBOLS}
    for prefix, want in by_prefix.items():
        assert {n for n in names if n.startswith(prefix)} == set(want), prefix
    assert (len(_lib.ASM_EXPORTED_SYMBOLS), len(_lib.OVL_EXPORTED_SYMBOLS), len(_lib.OVL_RULE_EXPORTED_SYMBOLS), len(_lib.RSETS_EXPORTED_SYMBOLS)) == (9, 9, 2, 17)
    # pgrc_match.h, pgrc_mem.h, pgrc_reads.h and the generators: the names _lib._PROTOS binds
    assert {n for n in names if re.match(r"pgrc_(match|synth|mem|divider)_", n)} == set(_lib.EXPORTED_SYMBOLS)
    # pgrc_decode.h: the decode context, the pair codings and the archive form
    decl = {p[0] for p in decode.DECODE_PROTOS}
    assert {n for n in names if re.match(r"pgrc_(decode|pairpos|pairorder|list_archive)_", n)} == decl
    # every exported name belongs to one of the headers' families
    fam = r"pgrc_(match|synth|mem|divider|decode|pairpos|pairorder|list_archive|asm|ovl|ovlrule|varlen|rsets|rlist)_"
    assert [n for n in names if not re.match(fam, n)] == ["pgrc_pg_alloc"]        # (the text allocator the adapters bind)
    # what the .hip files reach of one another stays hidden
    hidden = ("last_list", "pgovl_assemble", "device_resident", "mapping_device", "pg_order_resident", "resident_release", "la_encode_resident", "la_describe", "encode_joined", "pairpos_encode_device")
    assert not [n for n in names if any(h in n for h in hidden)]
    nm = subprocess.run(["nm", "-C", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "rocprim" not in nm                          # no library kernel


def test_layout_from_c(tmp_path):
    from pgrc_amd import _lib
    src = tmp_path / "rlist.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pgrc_readslist.h"', 'int main(void) {']
    for cname, pyname in STRUCTS.items():
        lines.append(f'    printf("%zu\\n", sizeof({cname}));')
        for f, _ in getattr(_lib, pyname)._fields_:
            lines.append(f'    printf("%zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname} *)0)->{f}));')
    lines += [f'    printf("%zu\\n", sizeof({c}));' for c in OLD_SIZES]
    lines += ['    printf("%d %d %d %d\\n", pgrc_rlist_create(0, NULL), pgrc_rlist_set_host(NULL, NULL), pgrc_rlist_pair_order(NULL, 0, NULL),',
              '           PGRC_RLIST_SET_HOST + 2 * PGRC_RLIST_ARCHIVE + 4 * PGRC_RLIST_PAIR_POSITIONS);',
              '    return 0;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "rlist"
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
    assert next(out).split() == ["1", "1", "1", "39"]


def test_null_arguments_are_refused_without_a_device():
    from pgrc_amd import _lib
    from pgrc_amd.decode import PairOrderStreams, PairPosStreams
    lib = _lib.lib
    assert lib.pgrc_rlist_create(0, None) == E_PARAM
    lib.pgrc_rlist_destroy(None)
    i, t, st, ar = _lib.RlistInfo(), _lib.RlistTiming(), _lib.ExportStreams(), _lib.RlistArchive()
    assert lib.pgrc_rlist_get_info(None, C.byref(i)) == E_PARAM and lib.pgrc_rlist_get_timing(None, C.byref(t)) == E_PARAM
    assert lib.pgrc_rlist_set_host(None, C.byref(st)) == E_PARAM and lib.pgrc_rlist_download(None, C.byref(st)) == E_PARAM
    assert lib.pgrc_rlist_from_assembly(None, None, None, 0) == E_PARAM
    assert lib.pgrc_rlist_from_overlap(None, None, None, None, 0, None) == E_PARAM
    assert lib.pgrc_rlist_export_pg_order(None, None, None) == E_PARAM
    assert lib.pgrc_rlist_archive_encode(None, 0, 0, C.byref(ar)) == E_PARAM
    lib.pgrc_rlist_archive_free(None)
    lib.pgrc_rlist_archive_free(C.byref(ar))            # an empty struct: nothing to give back
    assert bytes(ar) == bytes(C.sizeof(ar))
    po, pp = PairOrderStreams(), PairPosStreams()
    none = (C.c_void_p * 3)()
    assert lib.pgrc_rlist_pair_order(None, 0, C.byref(po)) == E_PARAM and lib.pgrc_rlist_pair_order(none, 0, C.byref(po)) == E_PARAM
    a = _lib.RlistPairPosArgs(C.sizeof(_lib.RlistPairPosArgs), 4, 0)
    assert lib.pgrc_rlist_pair_positions(None, C.byref(pp)) == E_PARAM and lib.pgrc_rlist_pair_positions(C.byref(a), C.byref(pp)) == E_PARAM
    assert isinstance(lib.pgrc_rlist_last_error(None), bytes)


def test_create_names_the_missing_device():
    """the reads list opens a stage handle of its own: without a device its create is PGRC_E_NO_DEVICE with the stage's text
    behind the list's prefix"""
    import torch
    from pgrc_amd import _lib
    if torch.cuda.is_available():
        return
    lib = _lib.lib
    h = C.c_void_p()
    assert lib.pgrc_rlist_create(-1, C.byref(h)) == 3 and not h.value
    assert lib.pgrc_rlist_last_error(None) == b"reads list: no HIP device"
