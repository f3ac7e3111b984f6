"""include/pgrc_verify.h: libpgrc_verify.so exports the header's seven names beside everything libpgrc_match.so exports, and
libpgrc_match.so exports none of them; the structs are laid out in pgrc_amd/_lib.py as the header lays them out (a C99 program
compiled with -pedantic -Werror prints sizes and offsets); NULL arguments are refused without a device; no library kernel is
linked.  No GPU: without a device there is no job, so pgrc_verify_begin cannot be reached (tests/test_gpu_verify.py has the
rest)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_PARAM = 1
STRUCTS = {"pgrc_verify_result": "VerifyResult", "pgrc_verify_timing": "VerifyTiming"}
SIZES = {"pgrc_verify_result": 112, "pgrc_verify_timing": 72}


def exported_names(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_symbols_are_exported_and_declared():
    from pgrc_amd import _lib
    names = exported_names(_lib.VERIFY_LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pgrc_verify.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*) ?(pgrc_verify_\w+)\(", header, flags=re.M))
    exported = {n for n in names if n.startswith("pgrc_verify_")}
    assert exported == declared == set(_lib.VERIFY_EXPORTED_SYMBOLS) and len(exported) == 7
    assert all(hasattr(_lib.vlib, s) for s in exported)
    # the library is the product's objects and verify.hip: every other name is libpgrc_match.so's, which has none of these
    base = exported_names(_lib.LIB_PATH)
    assert names - exported == base and not [n for n in base if "verify" in n]
    # what verify.hip and selftest.hip reach of one another and of the divider stays hidden
    assert not [n for n in names if "pgrc_vf_" in n or "last_reads_device" in n or "selftest" in n]
    nm = subprocess.run(["nm", "-C", _lib.VERIFY_LIB_PATH], capture_output=True, text=True).stdout
    assert "rocprim" not in nm and "k_vf_confirm" in nm         # no library kernel; its own kernels
    import pgrc_amd
    assert pgrc_amd.Verifier.__module__ == "pgrc_amd.verify"
    for m in ("add_rows", "add_fastq", "finish", "timing", "close"):
        assert callable(getattr(pgrc_amd.Verifier, m))
    assert callable(pgrc_amd.PgRCDecoder.verifier)


def test_layout_from_c(tmp_path):
    from pgrc_amd import _lib
    src = tmp_path / "verify.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pgrc_verify.h"', 'int main(void) {']
    for cname, pyname in STRUCTS.items():
        lines.append(f'    printf("%zu\\n", sizeof({cname}));')
        for f, _ in getattr(_lib, pyname)._fields_:
            lines.append(f'    printf("%zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname} *)0)->{f}));')
    lines += ['    printf("%d %d %d %d\\n", pgrc_verify_begin(NULL, 0, NULL), pgrc_verify_add_rows(NULL, 0, NULL, 0), pgrc_verify_finish(NULL, NULL),',
              '           PGRC_VERIFY_AUTO + 2 * PGRC_VERIFY_IN_ORDER + 4 * PGRC_VERIFY_MULTISET);',
              '    printf("%llu\\n", (unsigned long long)PGRC_VERIFY_MAX_ITEMS);',
              '    return 0;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "verify"
    libdir = os.path.dirname(_lib.VERIFY_LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lpgrc_verify", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = iter(subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n"))
    for cname, pyname in STRUCTS.items():
        st = getattr(_lib, pyname)
        assert int(next(out)) == C.sizeof(st) == SIZES[cname], cname
        for f, _ in st._fields_:
            off, size = (int(x) for x in next(out).split())
            d = getattr(st, f)
            assert (d.offset, d.size) == (off, size), (cname, f)
    assert next(out).split() == ["1", "1", "1", "10"]
    assert int(next(out)) == 0x7FFFF800


def test_null_arguments_are_refused_without_a_device():
    from pgrc_amd import _lib
    lib = _lib.vlib
    h = C.c_void_p()
    assert lib.pgrc_verify_begin(None, 0, None) == E_PARAM
    assert lib.pgrc_verify_begin(None, 0, C.byref(h)) == E_PARAM and not h
    assert b"job is NULL" in lib.pgrc_verify_last_error(None)
    n = C.c_uint64(0)
    assert lib.pgrc_verify_add_rows(None, 0, None, 0) == E_PARAM
    assert lib.pgrc_verify_add_fastq(None, None, 0, None, 0, 1, C.byref(n), None, C.byref(n)) == E_PARAM
    r, t = _lib.VerifyResult(), _lib.VerifyTiming()
    assert lib.pgrc_verify_finish(None, C.byref(r)) == E_PARAM and lib.pgrc_verify_get_timing(None, C.byref(t)) == E_PARAM
    lib.pgrc_verify_end(None)
