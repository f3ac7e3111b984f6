"""CPU check of the numpy restatements of the Pg-vs-Pg marking and its inverse (tests/pgmap_util.py) against fixtures
the real reference made (tests/golden/make_golden_pgmap.py): markAndRemoveExactMatches from the reference's own raw
matches reproduces its mapped bytes and streams exactly, and the serial restoreMatchedPg turns them back into the
original texts."""
import glob
import hashlib
import os

import numpy as np
import pytest

import pgmap_util as pu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "pgmap_*.npz")))


def load_case(path):
    z = np.load(path)
    seed, G, Gl, Gn, nrep, chains, depth, lowc, tl = (int(x) for x in z["params"])
    texts = pu.make_texts(seed, G, Gl, Gn, nrep=nrep, chains=chains, chain_depth=depth, low_complexity=bool(lowc))
    for p, t in enumerate(texts):
        assert hashlib.sha256(t.tobytes()).hexdigest()[:16] == z[f"digest{p}"].tobytes().decode(), "text generator drifted"
    return z, texts, tl


def test_fixtures_present():
    names = {os.path.basename(f) for f in FIXTURES}
    assert {"pgmap_hq_lq_n.npz", "pgmap_empty_n.npz", "pgmap_short_hq.npz", "pgmap_low_complexity.npz",
            "pgmap_rc_chains.npz"} <= names


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[6:-4])
def test_mark_and_remove_matches_the_reference(path):
    z, texts, tl = load_case(path)
    hq = texts[0]
    for p, dest in enumerate(texts):
        if hq.size < tl:
            got = (dest.tobytes(),) + pu.no_matcher_streams()
        else:
            got = pu.mark_and_remove(dest, z[f"matches{p}"], p == 0, True, tl, hq.size)
        for k, g in zip(("mapped", "off", "len"), got):
            assert g == z[f"{k}{p}"].tobytes(), f"part {p}: {k} differs"


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[6:-4])
def test_serial_restore_gives_the_texts_back(path):
    z, texts, _ = load_case(path)
    mapped = b"".join(z[f"mapped{p}"].tobytes() for p in range(3))
    lens = [z[f"mapped{p}"].size for p in range(3)]
    got = pu.restore_matched_pgs(mapped, lens, texts[0].size, [z[f"off{p}"].tobytes() for p in range(3)],
                                 [z[f"len{p}"].tobytes() for p in range(3)])
    for p in range(3):
        assert got[p] == texts[p].tobytes()


def test_byte_frugal_round_trip_and_widths():
    vals = [0, 1, 127, 128, 16383, 16384, 2**32 - 1, 2**32, 2**63, 2**64 - 1]
    s = pu.frugal_stream(vals)
    at, back = 0, []
    for _ in vals:
        v, at = pu.read_uint_byte_frugal(s, at)
        back.append(v)
    assert back == vals and at == len(s)
    assert len(pu.frugal_stream([2**64 - 1])) == 10
    # 8-byte offsets above 2^32 symbols of HQ
    m, off, ln = pu.build_part([b"ACGT", (1, 3)], min_len=2, width=8)
    assert m == b"ACGT%" and len(off) == 8 and ln == bytes([2, 1])


def test_hop_classes_of_the_serial_restore():
    # c(c(x)) is not x for lower case, U, or bytes outside complementsLut: a restore restatement that treats an even
    # number of hops as the identity gets these wrong
    lit = b"acgtuRYkmbdhvnN#"
    n = len(lit)
    hq_m, hq_o, hq_l = pu.build_part([lit, (0, n), (n, n), (2 * n, n)], min_len=0)
    hq = pu.restore_matched_pg(b"", n * 4, hq_m, hq_o, hq_l, True, True)
    one = pu.reverse_complement(lit)
    two = pu.reverse_complement(one)
    assert hq == lit + one + two + pu.reverse_complement(two)
    assert two != lit
