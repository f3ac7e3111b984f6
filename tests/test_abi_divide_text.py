"""include/pgrc_reads.h and include/pgrc_reads_text.h: the text entries for FASTA and one-read-per-line sources.  The headers
compile as strict C99; pgrc_divider_run_text is exported by every library beside pgrc_divider_run_fastq;
pgrc_reads_text_format and pgrc_verify_add_text are libpgrc_reads_text.so's alone, which otherwise exports what
libpgrc_verify.so exports; the format choice is the reference's; what is refused before the device is touched is refused
without one.  No GPU: without a device there is no divider, so the refusals that need a handle are in
tests/test_gpu_divide_text.py."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_PARAM = 1


def exported_names(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_names_are_exported_where_the_headers_say():
    from pgrc_amd import _lib
    base, verify, text = exported_names(_lib.LIB_PATH), exported_names(_lib.VERIFY_LIB_PATH), exported_names(_lib.READS_TEXT_LIB_PATH)
    for names in (base, verify, text, exported_names(_lib.RLIST_ORD_LIB_PATH)):
        assert {"pgrc_divider_run_text", "pgrc_divider_run_fastq"} <= names
    assert "pgrc_divider_run_text" in _lib.EXPORTED_SYMBOLS
    own = set(_lib.READS_TEXT_EXPORTED_SYMBOLS)
    assert own == {"pgrc_reads_text_format", "pgrc_verify_add_text"}
    assert text - verify == own and verify <= text and not own & base
    assert not [n for n in text if "pgrc_vf_" in n]                    # what readstext.hip reaches of verify.hip stays hidden
    import pgrc_amd
    assert callable(pgrc_amd.DividedPCLReadsSets.divide_text) and callable(pgrc_amd.Verifier.add_text)
    assert callable(pgrc_amd.reads_text_format)


def test_format_by_the_first_byte():
    from pgrc_amd import _lib, reads_text_format
    f = _lib.tlib.pgrc_reads_text_format
    want = {ord("@"): 0, ord(">"): 1, ord(";"): 1, ord("A"): 2, ord("\n"): 2, -1: 2}
    for byte, fmt in want.items():
        assert f(byte) == fmt == reads_text_format(byte), byte
    assert reads_text_format(b"@r1\nACGT\n") == 0 and reads_text_format(b";c\n>r\nAC\n") == 1 and reads_text_format(b"") == 2
    assert (_lib.READS_FASTQ, _lib.READS_FASTA, _lib.READS_LINES) == (0, 1, 2)
    assert [_lib.reads_format(x) for x in ("fastq", "FASTA", "lines", 2)] == [0, 1, 2, 2]


def test_headers_are_plain_c99_and_link_from_c(tmp_path):
    from pgrc_amd import _lib
    src = tmp_path / "text.c"
    src.write_text("\n".join([
        '#include <stdio.h>', '#include "pgrc_reads_text.h"', 'int main(void) {',
        '    uint64_t used = 0, n = 0;', '    pgrc_divided_reads out;',
        '    int a = pgrc_divider_run_text(NULL, PGRC_READS_FASTA, NULL, 0, NULL, 0, 0, 1, &used, NULL, &n, &out);',
        '    int b = pgrc_divider_run_text(NULL, PGRC_READS_LINES, NULL, 0, NULL, 0, 0, 1, &used, NULL, &n, &out);',
        '    int c = pgrc_divider_run_text(NULL, PGRC_READS_FASTQ, NULL, 0, NULL, 0, 0, 1, &used, NULL, &n, &out);',
        '    int d = pgrc_divider_run_text(NULL, 7, NULL, 0, NULL, 0, 0, 1, &used, NULL, &n, &out);',
        '    int e = pgrc_verify_add_text(NULL, PGRC_READS_FASTA, NULL, 0, NULL, 0, 1, &used, NULL, &n);',
        "    printf(\"%d %d %d %d %d %d %d %d\\n\", a, b, c, d, e, pgrc_reads_text_format('@'), pgrc_reads_text_format(';'), pgrc_reads_text_format(-1));",
        '    printf("%d %d %d\\n", PGRC_READS_FASTQ, PGRC_READS_FASTA, PGRC_READS_LINES);', '    return 0;', '}']) + "\n")
    exe = tmp_path / "text"
    libdir = os.path.dirname(_lib.READS_TEXT_LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lpgrc_reads_text", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n")
    assert out[0].split() == ["1", "1", "1", "1", "1", "0", "1", "2"] and out[1].split() == ["0", "1", "2"]
    # pgrc_reads.h alone, against the product library
    src.write_text('#include "pgrc_reads.h"\nint main(void) { return pgrc_divider_run_text(NULL, PGRC_READS_LINES, NULL, 0, NULL, 0, 0, 1, NULL, NULL, NULL, NULL) != 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lpgrc_match", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


def test_refusals_in_front_of_the_device():
    """a NULL handle or NULL results are PGRC_E_PARAM in every format, an unknown format too: nothing of it needs a device"""
    from pgrc_amd import _lib
    used, n, out = C.c_uint64(7), C.c_uint64(7), _lib.DividedReads()
    run = _lib.lib.pgrc_divider_run_text
    for fmt in (0, 1, 2, 7, -1):
        assert run(None, fmt, None, 0, None, 0, 0, 1, C.byref(used), None, C.byref(n), C.byref(out)) == E_PARAM
        assert _lib.tlib.pgrc_verify_add_text(None, fmt, None, 0, None, 0, 1, C.byref(used), None, C.byref(n)) == E_PARAM
    assert (used.value, n.value) == (7, 7)
