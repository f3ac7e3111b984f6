"""The round skip of the dual kernel (pgrc_amd/csrc/dualkern.h, "Round skip"), checked on the CPU: tests/roundskip_model.py
restates the reference's per-read query with the skip schedule and its rewind; positions, strands and counts must equal
the oracle's (early-stop restatement of CopMEMMatcher.cpp:483-566) on every input, while the probed seeds must not rise."""
import numpy as np
import pytest

import oracle as orc
import roundskip_model as rsm
from test_early_stop_rule import CASES
from util import make_inputs

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _check(pg, reads, seed_len, kmax, kmin):
    ref = orc.oracle_match("c", pg, reads, seed_len, kmax, kmin, True, early_stop=True)
    strands = (rsm.Strand(pg, seed_len), rsm.Strand(rsm.revcomp(np.ascontiguousarray(pg, dtype=np.uint8)), seed_len))
    plain, sp = rsm.match_two_pass(pg, reads, seed_len, kmax, kmin, False, strands)
    skip, ss = rsm.match_two_pass(pg, reads, seed_len, kmax, kmin, True, strands)
    for k in ("pos", "rc", "mism"):
        assert np.array_equal(np.asarray(ref[k]), plain[k]), ("model without the skip", k)
        assert np.array_equal(np.asarray(ref[k]), skip[k]), ("round skip", k, np.flatnonzero(np.asarray(ref[k]) != skip[k])[:10])
    assert ref["matched"] == skip["matched"]
    assert ss.probes <= sp.probes + 2 * ss.rewinds * reads.shape[1]   # (a rewind re-probes at most a read's seeds)
    return sp, ss


@pytest.mark.parametrize("L,seed_len,M,kmin_is_kmax,G,n,pool_div,tandem", CASES)
def test_round_skip_changes_nothing(L, seed_len, M, kmin_is_kmax, G, n, pool_div, tandem):
    pg, reads = make_inputs(G, n, L, seed=L * 1000 + seed_len + M, pool_div=pool_div, tandem_every=tandem)
    kmax = L // M
    _check(pg, reads, seed_len, kmax, kmax if kmin_is_kmax else 0)


def _low_complexity(unit_len, seed):
    rng = np.random.default_rng(seed)
    unit = rng.choice(_ACGT, size=unit_len)
    pg = np.tile(unit, 100000 // unit_len + 1)[:100000].copy()
    flips = rng.integers(0, pg.size, size=600)
    pg[flips] = rng.choice(_ACGT, size=flips.size)
    _, reads = make_inputs(100000, 800, 100, seed=seed)
    for i, st in enumerate(rng.integers(0, pg.size - 100, size=600)):
        reads[i] = pg[st:st + 100]
        for _ in range(int(rng.integers(0, 5))):
            reads[i, int(rng.integers(0, 100))] = rng.choice(_ACGT)
    return pg, reads


@pytest.mark.parametrize("unit_len", [37, 7])
def test_round_skip_on_low_complexity_and_capped_buckets(unit_len):
    """Repeats: buckets at the 13-entry cap (dirty rounds inside skip mode), reads whose falses budget runs out, and
    acceptable alignments met first in skip mode (rewinds)."""
    pg, reads = _low_complexity(unit_len, 5 + unit_len)
    for kmax in (2, 5, 33):
        sp, ss = _check(pg, reads, 38, kmax, 0)
        assert ss.skipped > 0


def test_round_skip_random_sweep():
    rng = np.random.default_rng(2024)
    for _ in range(12):
        L = int(rng.integers(40, 256))
        seed_len = int(rng.integers(24, min(L, 140) + 1))
        kmax = min(L // int(rng.choice([1000, 60, 50, 25, 10, 4])), 247)
        pg, reads = make_inputs(int(rng.integers(L + 50, 150000)), int(rng.integers(1, 1500)), L,
                                seed=int(rng.integers(0, 1 << 30)), pool_div=int(rng.choice([8, 64])),
                                tandem_every=int(rng.choice([0, 2, 64])))
        _check(pg, reads, seed_len, kmax, kmax if rng.random() < 0.25 else 0)


def test_round_skip_rewinds_happen():
    pg, reads = make_inputs(200000, 1500, 150, seed=77, tandem_every=2)
    _, ss = _check(pg, reads, 38, 3, 0)
    assert ss.skipped > 0 and ss.rewinds > 0


def c3_estimate(n=3000, G=4_000_000):
    """Probed seeds per read at C3's L / seed / M (150 / 38 / 50) under both schedules, the reference's two passes."""
    pg, reads = make_inputs(G, n, 150, seed=12345, tandem_every=64)
    strands = (rsm.Strand(pg, 38), rsm.Strand(rsm.revcomp(pg), 38))
    _, sp = rsm.match_two_pass(pg, reads, 38, 3, 0, False, strands)
    _, ss = rsm.match_two_pass(pg, reads, 38, 3, 0, True, strands)
    return sp, ss, n


if __name__ == "__main__":
    sp, ss, n = c3_estimate()
    print(f"C3 shape (L 150, seed 38, -M 50, two passes), {n} reads: seeds probed per read {sp.probes / n:.2f} without the "
          f"round skip, {ss.probes / n:.2f} with it ({1 - ss.probes / sp.probes:.1%} fewer); skipping queries {ss.skipped / n:.3f} "
          f"per read, rewinds {ss.rewinds / n:.3f} per read")
