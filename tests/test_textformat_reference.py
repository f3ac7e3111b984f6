"""tests/textformat_util.py's restatement of the FASTA and one-read-per-line iterators against the compiled reference: the
restatement's rows, divided by the oracle division, equal what the reference's managed iterator (which picks the format by the
file's first byte) and its factory make of the same files.  Shows that the files the GPU tests use are files the reference
itself accepts.  No GPU."""
import numpy as np
import pytest

import oracle as orc
import textformat_util as tu
from divide_util import COMBOS, make_records, oracle_divide, ref_divide_files, same

HAVE_REF = orc.have_ref() and hasattr(orc.ref(), "pgrc_ref_divide_files")
pytestmark = pytest.mark.skipif(not HAVE_REF, reason="needs oracle/_ref")

N = 200
PLAIN = [c for c in COMBOS if c[0] >= 1]             # no qualities in these formats


def check(tmp_path, fmt, a, b, rev, L):
    (tmp_path / "a.txt").write_bytes(a)
    if b is not None:
        (tmp_path / "b.txt").write_bytes(b)
    rows = tu.restate(fmt, a, b, rev, L)
    assert isinstance(rows, np.ndarray)
    for combo in PLAIN:
        want = ref_divide_files(tmp_path / "a.txt", tmp_path / "b.txt" if b is not None else None, rev, L, N + 8, combo)
        assert want["n_hq"] + want["n_lq"] + want["n_n"] == rows.shape[0]
        got = oracle_divide(rows, None, *combo)
        assert same(got, want) is None, (combo, same(got, want))
    return rows.shape[0]


@pytest.mark.parametrize("L", [21, 100])
def test_fasta_single(tmp_path, L):
    reads, _ = make_records(seed=L, n=N, L=L)
    assert check(tmp_path, tu.FASTA, tu.write_fasta(reads, seed=1), None, False, L) == N
    every = tu.write_fasta(reads, seed=2, crlf=True, trailing_newline=False, comments=True, multi_headers=True, header_last=True, tail_text=True)
    assert every[:1] == b";" and not every.endswith(b"\n")
    assert check(tmp_path, tu.FASTA, every, None, False, L) == N
    assert check(tmp_path, tu.FASTA, tu.write_fasta(reads, seed=3, trailing_newline=False), None, False, L) == N


@pytest.mark.parametrize("L", [21, 100])
@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("n_a,n_b", [(N // 2, N // 2), (N // 2, N // 2 - 1), (N // 2 - 1, N // 2)])
def test_fasta_pair(tmp_path, L, rev, n_a, n_b):
    reads, _ = make_records(seed=L + 7, n=N, L=L)
    a = tu.write_fasta(reads[0::2][:n_a], seed=1, comments=True)
    b = tu.write_fasta(reads[1::2][:n_b], seed=2, multi_headers=True, header_last=True)
    # the reference stops at the first exhausted file: when its turn comes
    assert check(tmp_path, tu.FASTA, a, b, rev, L) == (2 * n_a if n_a <= n_b else 2 * n_b + 1)


@pytest.mark.parametrize("L", [21, 100])
def test_lines_single(tmp_path, L):
    reads, _ = make_records(seed=L + 3, n=N, L=L)
    assert check(tmp_path, tu.LINES, tu.write_lines(reads), None, False, L) == N
    assert check(tmp_path, tu.LINES, tu.write_lines(reads, crlf=True, trailing_newline=False, tail_text=True), None, False, L) == N


def test_lines_ignore_a_pair_file(tmp_path):
    """the reference hands ConcatenatedReadsSourceIterator no second stream: the pair file is never read (the library
    refuses the combination instead, include/pgrc_reads.h)"""
    reads, _ = make_records(seed=5, n=N, L=40)
    assert check(tmp_path, tu.LINES, tu.write_lines(reads[:60]), tu.write_lines(reads[60:]), False, 40) == 60
