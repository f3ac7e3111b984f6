"""tests/handover_util.py's numpy references of the hand-over formats against what exists already: the row packers equal the
oracle's pgrc_or_pack_read (which tests/test_oracle_vs_ref.py pins to the compiled reference) byte for byte at every read
length, the text packer and the reverse complement equal util.pack2 and util.revcomp at every G mod 16, and the word array,
the flags and the position bytes unpack to the ASCII rows they were made from.  No GPU."""
import subprocess

import numpy as np
import pytest

import handover_util as hu
from util import pack2, pack_rows, revcomp


def random_rows(rng, n, L, n_rate):
    """n rows of L symbols; a third of the rows hold N's at rate n_rate, one row is all N, one has a single N at the end"""
    rows = hu.ASCII[rng.integers(0, 4, (n, L), dtype=np.uint8)]
    if n_rate:
        with_n = rng.random(n) < 1 / 3
        rows[(rng.random((n, L)) < n_rate) & with_n[:, None]] = hu.N
        rows[0] = hu.N
        rows[1, L - 1] = hu.N
    return rows


@pytest.mark.parametrize("block", range(5))
def test_row_packers_equal_the_oracle_at_every_read_length(block):
    rng = np.random.default_rng(50 + block)
    for L in range(1 + 51 * block, 1 + 51 * (block + 1)):
        rows = random_rows(rng, 36, L, 0)
        codes, nmask = hu.symbols(rows)
        assert not nmask.any()
        assert np.array_equal(hu.acgt_bytes(codes), pack_rows(rows)), f"ACGT bytes, L = {L}"
        assert np.array_equal(hu.rows_of(rows, 4), pack_rows(rows))
        rows = random_rows(rng, 36, L, 0.08)
        codes, nmask = hu.symbols(rows)
        assert nmask.any()
        assert np.array_equal(hu.acgnt_bytes(codes, nmask), pack_rows(rows, b"ACGNT")), f"ACGNT bytes, L = {L}"
        assert np.array_equal(hu.ascii_rows(codes, nmask), rows)


def test_text_packer_and_reverse_complement_equal_util_at_every_residue():
    rng = np.random.default_rng(7)
    for G in list(range(1, 81)) + [4095, 4096, 4097, 65543]:
        pg = hu.ASCII[rng.integers(0, 4, G, dtype=np.uint8)]
        assert np.array_equal(hu.pack_text(pg), pack2(pg)), G
        assert np.array_equal(hu.revcomp_text(pg), pack2(revcomp(pg))), G


@pytest.mark.parametrize("block", range(5))
def test_words_flags_and_positions_unpack_to_the_rows(block):
    rng = np.random.default_rng(90 + block)
    for L in range(1 + 51 * block, 1 + 51 * (block + 1)):
        rows = random_rows(rng, 40, L, 0.02)
        st = hu.read_state(rows)
        cnt = (rows == hu.N).sum(axis=1)
        assert np.array_equal(st["flag"], np.where(cnt == 0, 0, np.where(cnt <= 4, 3, 1))), L
        back = hu.unpack_reads(st["words"], st["flag"], st["npos"], L)
        few = st["flag"] != 1
        assert np.array_equal(back[few], rows[few]), L
        many = ~few                                     # their N's are kept in the side list only: code 0 in the words
        assert np.array_equal(back[many], np.where(rows[many] == hu.N, ord("A"), rows[many])), L
        assert np.array_equal(st["nidx"], np.flatnonzero(cnt)) and np.array_equal(st["nascii"], rows[cnt > 0]), L
        assert st["n_many"] == int((cnt > 4).sum())
        # the literal rule of the position word: the first four N's, lowest first, 0xFF for none
        for r in np.flatnonzero(st["flag"] == 3):
            at = [i for i in range(L) if rows[r, i] == hu.N]
            assert [int(st["npos"][r]) >> (8 * k) & 0xFF for k in range(4)] == at + [0xFF] * (4 - len(at)), (L, r)


def test_selftest_entries_stay_out_of_the_product_library():
    """the hand-over entries are in libpgrc_selftest.so alone (the style of tests/test_abi.py)"""
    from pgrc_amd import _lib
    import prim_util as pu

    def names(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    product = names(_lib.LIB_PATH)
    assert product and not [s for s in product if s.startswith("pgrc_selftest_")]
    assert {"pgrc_selftest_pack_text", "pgrc_selftest_revcomp", "pgrc_selftest_pack_reads", "pgrc_selftest_nrows_ascii",
            "pgrc_selftest_reads_state"} <= names(pu.LIB_PATH)
