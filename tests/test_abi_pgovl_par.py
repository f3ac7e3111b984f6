"""The rule of the sweeps in include/pgrc_overlap.h (pgrc_ovl_set_rule, pgrc_ovl_get_rule_info): the two entry points are
exported by the library and declared in the Python mirror, the header's names for them compile and link from C99,
pgrc_ovl_rule_info is laid out in pgrc_amd/_lib.py as the header lays it out, and the structs the header had before keep their
sizes.  No GPU: without a device pgrc_ovl_create fails, so of the parameter errors only the ones in front of it are asserted
here (tests/test_gpu_pgovl_par.py has the rest)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pgrc_ovlrule_set", "pgrc_ovlrule_get_info")
HEADER_NAMES = {"pgrc_ovl_set_rule": "pgrc_ovlrule_set", "pgrc_ovl_get_rule_info": "pgrc_ovlrule_get_info"}
FIELDS = ("struct_size", "rule", "blocks", "tail_sweeps", "follower_compares", "past_end_compares")
OLD_SIZES = {"pgrc_ovl_input": 48, "pgrc_ovl_result": 64, "pgrc_ovl_timing": 56}


def test_symbols_are_exported_and_declared():
    from pgrc_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "pgrc_overlap.h")).read()
    for s in SYMBOLS:
        assert s in names, f"{s} is not exported"
        assert s in _lib.OVL_RULE_EXPORTED_SYMBOLS and hasattr(_lib.lib, s)
        assert s + "(" in header
    assert {n for n in names if n.startswith("pgrc_ovlrule_")} == set(SYMBOLS) == set(_lib.OVL_RULE_EXPORTED_SYMBOLS)
    for name, symbol in HEADER_NAMES.items():
        assert f"#define {name} {symbol}\n" in header
    assert "The parallel generator of -t > 1" not in header and "avoidCyclesMode is not covered" in header
    assert _lib.OVL_RULES == {"serial": 0, "parallel": 1}


def test_layout_and_the_headers_names_from_c(tmp_path):
    from pgrc_amd import _lib
    src = tmp_path / "rule.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pgrc_overlap.h"', 'int main(void) {',
             '    pgrc_ovl_rule_info info;',
             '    printf("%zu\\n", sizeof(pgrc_ovl_rule_info));']
    lines += [f'    printf("%zu %zu\\n", offsetof(pgrc_ovl_rule_info, {f}), sizeof(((pgrc_ovl_rule_info *)0)->{f}));' for f in FIELDS]
    lines += [f'    printf("%zu\\n", sizeof({c}));' for c in OLD_SIZES]
    lines += ['    info.struct_size = sizeof(info);',
              '    printf("%d %d %d\\n", pgrc_ovl_set_rule(NULL, PGRC_OVL_RULE_PARALLEL), pgrc_ovl_get_rule_info(NULL, &info), (int)(PGRC_OVL_RULE_SERIAL + 2 * PGRC_OVL_RULE_PARALLEL));',
              '    return 0;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "rule"
    libdir = os.path.dirname(_lib.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lpgrc_match", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = iter(subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n"))
    st = _lib.OvlRuleInfo
    assert int(next(out)) == C.sizeof(st) == 32
    assert [f for f, _ in st._fields_] == list(FIELDS)
    for f in FIELDS:
        off, size = (int(x) for x in next(out).split())
        d = getattr(st, f)
        assert (d.offset, d.size) == (off, size), f
    for cname, size in OLD_SIZES.items():
        assert int(next(out)) == size, cname
    assert next(out).split() == ["1", "1", "2"]            # PGRC_E_PARAM twice: a NULL context


def test_null_arguments_are_refused_without_a_device():
    from pgrc_amd import _lib
    lib = _lib.lib
    assert lib.pgrc_ovlrule_set(None, 0) == 1 and lib.pgrc_ovlrule_set(None, 1) == 1 and lib.pgrc_ovlrule_set(None, 2) == 1
    assert lib.pgrc_ovlrule_get_info(None, None) == 1
    info = _lib.OvlRuleInfo(C.sizeof(_lib.OvlRuleInfo))
    assert lib.pgrc_ovlrule_get_info(None, C.byref(info)) == 1
    assert C.sizeof(_lib.OvlInput) == 48 and C.sizeof(_lib.OvlResult) == 64 and C.sizeof(_lib.OvlTiming) == 56


def test_the_wrapper_refuses_an_unknown_rule_before_any_call():
    import pytest
    from pgrc_amd import OverlapFinder
    ovl = OverlapFinder.__new__(OverlapFinder)              # (no context: the name is checked first)
    ovl._h = C.c_void_p()
    with pytest.raises(ValueError):
        ovl.set_rule("threads")
