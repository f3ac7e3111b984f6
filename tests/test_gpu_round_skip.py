"""The round skip of the dual kernel (pgrc_amd/csrc/dualkern.h, "Round skip") on the device: results with the skip on
(the default) equal the oracle's and those of PGRC_ROUND_SKIP=0, on inputs that make the kernel skip, rewind, meet
dirty rounds in skip mode, carry N's, continue an earlier phase and come in pairs.  The counters must show that skip
mode and rewinds happened."""
import numpy as np
import pytest

import oracle as orc
from util import assert_same_results, make_inputs, revcomp

pytestmark = pytest.mark.gpu

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _run(monkeypatch, pg, reads, seed_len, kmax, skip, state=None):
    from pgrc_amd import MatchContext
    monkeypatch.setenv("PGRC_DUAL", "1")
    monkeypatch.setenv("PGRC_ROUND_SKIP", skip)
    ctx = MatchContext(reads.shape[1], seed_len, kmax, 0, "c")
    ctx.set_pg_ascii(pg)
    ctx.set_reads_ascii(reads)
    ctx.set_profiling(True)
    if state is None:
        ctx.init_results()
    else:
        ctx.set_results(*[np.ascontiguousarray(a) for a in state])
    ctx.run(True)
    pos, rc, mism, hist, matched = ctx.get_results()
    c = ctx.counters()
    ctx.close()
    return {"pos": pos, "rc": rc, "mism": mism, "hist": hist, "matched": matched}, c


def _both(monkeypatch, pg, reads, seed_len, kmax, state=None):
    o = orc.oracle_match("c", pg, reads, seed_len, kmax, 0, state=state)
    on, c_on = _run(monkeypatch, pg, reads, seed_len, kmax, "1", state)
    off, c_off = _run(monkeypatch, pg, reads, seed_len, kmax, "0", state)
    assert c_on["screened"] == 2 and c_off["screened"] == 2           # (the dual kernel ran)
    assert_same_results(on, o, "round skip vs oracle")
    assert_same_results(off, o, "no round skip vs oracle")
    assert c_off["dual_skip_reads"] == 0 and c_off["dual_rewinds"] == 0
    assert c_on["dual_seed_probes"] <= c_off["dual_seed_probes"] + 2 * c_on["dual_rewinds"] * reads.shape[1]
    return c_on, c_off


def _plant(pg, rng, reads, rows, L, mism_at, from_rc):
    """reads[rows] = text windows (or their reverse complements) with a mismatch at each symbol of mism_at"""
    for i in rows:
        st = int(rng.integers(0, pg.size - L))
        r = pg[st:st + L].copy()
        if from_rc:
            r = revcomp(r)
        for x in mism_at:
            r[x] = _ACGT[(np.flatnonzero(_ACGT == r[x])[0] + 1 + int(rng.integers(0, 3))) % 4]
        reads[i] = r


def test_round_skip_rewinds_and_finishes_in_skip_mode(monkeypatch):
    """L 150, seed 38 (K 28, k1 5, k2 2: rounds of seeds 0-4, 15-19, ...).  A mismatch at symbol 20 spoils every
    round-0 window of the alignment's class, so it shows first at a seed between rounds 0 and 1 (skipped): the lane
    meets it in round 1 and rewinds.  Reads with two or three mismatches after the first round's windows are accepted
    at once and then finish in skip mode."""
    L = 150
    rng = np.random.default_rng(11)
    pg, reads = make_inputs(400_000, 6000, L, seed=311, pool_div=32)
    _plant(pg, rng, reads, range(0, 600), L, [20], False)
    _plant(pg, rng, reads, range(600, 1200), L, [20, 120], True)
    _plant(pg, rng, reads, range(1200, 1800), L, [60, 140], False)               # m = 2
    _plant(pg, rng, reads, range(1800, 2400), L, [50, 90, 130], True)            # m = 3
    for kmax in (3, 5):
        c_on, c_off = _both(monkeypatch, pg, reads, 38, kmax)
        assert c_on["dual_skip_reads"] > 1000 and c_on["dual_rewinds"] > 300
        assert c_on["dual_seed_probes"] < c_off["dual_seed_probes"]


@pytest.mark.parametrize("unit_len", [37, 7])
def test_round_skip_dirty_rounds_in_skip_mode(monkeypatch, unit_len):
    """Low-complexity text: buckets at the 13-entry cap make rounds in skip mode dirty; reads whose falses budget runs
    out (redo in the reference's order) and repeats with many equal alignments."""
    rng = np.random.default_rng(unit_len)
    unit = rng.choice(_ACGT, size=unit_len)
    pg = np.tile(unit, 200_000 // unit_len + 1)[:200_000].copy()
    flips = rng.integers(0, pg.size, size=1500)
    pg[flips] = rng.choice(_ACGT, size=flips.size)
    _, reads = make_inputs(200_000, 4000, 100, seed=unit_len)
    for i, st in enumerate(rng.integers(0, pg.size - 100, size=3000)):
        reads[i] = pg[st:st + 100]
        for _ in range(int(rng.integers(0, 5))):
            reads[i, int(rng.integers(0, 100))] = rng.choice(_ACGT)
    for kmax in (2, 5):
        c_on, _ = _both(monkeypatch, pg, reads, 38, kmax)
        assert c_on["dual_skip_reads"] > 0


def test_round_skip_reads_with_ns(monkeypatch):
    """Reads with 1-4 N's are the dual kernel's own; an N in the windows of round 0 forces rewinds as a mismatch does."""
    L = 150
    rng = np.random.default_rng(12)
    pg, reads = make_inputs(400_000, 5000, L, seed=312, pool_div=32)
    _plant(pg, rng, reads, range(0, 2000), L, [], False)
    N = ord("N")
    for i in range(2000):
        k = 1 + i % 4
        xs = [20] + [int(x) for x in rng.choice(np.arange(40, L), size=k - 1, replace=False)] if i % 2 else \
            [int(x) for x in rng.choice(L, size=k, replace=False)]
        reads[i, xs] = N
    c_on, _ = _both(monkeypatch, pg, reads, 38, 5)
    assert c_on["dual_skip_reads"] > 0 and c_on["dual_rewinds"] > 0


def test_round_skip_two_phase_continuation(monkeypatch):
    """A read's count before the run (cin) and its starting limit L0 come from an earlier phase."""
    L = 150
    rng = np.random.default_rng(13)
    pg, reads = make_inputs(400_000, 5000, L, seed=313, pool_div=32)
    _plant(pg, rng, reads, range(0, 1000), L, [20], False)
    _plant(pg, rng, reads, range(1000, 2000), L, [20, 70, 110], True)
    first = orc.oracle_match("c", pg, reads, 38, 2, 0, rev_compl=False)
    state = (first["pos"], first["rc"], first["mism"])
    assert (first["mism"] != 255).any() and (first["mism"] > 0).any()
    c_on, _ = _both(monkeypatch, pg, reads, 38, 5, state=state)
    assert c_on["dual_skip_reads"] > 0 and c_on["dual_rewinds"] > 0


def test_round_skip_paired_reads(monkeypatch):
    L = 150
    pg, reads = make_inputs(400_000, 6000, L, seed=314, paired=True, pool_div=32)
    rng = np.random.default_rng(14)
    _plant(pg, rng, reads, range(0, 6000, 7), L, [20], False)
    c_on, _ = _both(monkeypatch, pg, reads, 38, 3)
    assert c_on["dual_skip_reads"] > 0 and c_on["dual_rewinds"] > 0


def test_unsized_counters_getter_keeps_the_older_layout(monkeypatch):
    """pgrc_match_counters grew at its end (the two round-skip counters): pgrc_match_get_counters writes only the struct
    that a caller built before that holds, and pgrc_match_get_counters_sized brings the new fields."""
    import ctypes as C
    from pgrc_amd import _lib
    pg, reads = make_inputs(200_000, 3000, 150, seed=315, pool_div=32)
    _plant(pg, np.random.default_rng(15), reads, range(0, 600), 150, [20], False)
    from pgrc_amd import MatchContext
    monkeypatch.setenv("PGRC_DUAL", "1")
    ctx = MatchContext(150, 38, 3, 0, "c")
    ctx.set_pg_ascii(pg)
    ctx.set_reads_ascii(reads)
    ctx.set_profiling(True)
    ctx.init_results()
    ctx.run(True)
    base = _lib.Counters.dual_skip_reads.offset
    buf = (C.c_uint8 * (C.sizeof(_lib.Counters) + 64))(*([0xAB] * (C.sizeof(_lib.Counters) + 64)))
    assert _lib.lib.pgrc_match_get_counters(ctx._h, C.cast(buf, C.POINTER(_lib.Counters))) == 0
    assert all(b == 0xAB for b in bytes(buf)[base:])                 # nothing written past the older struct
    old = _lib.Counters.from_buffer_copy(bytes(buf)[:C.sizeof(_lib.Counters)])
    c = ctx.counters()
    assert old.screened == 2 and old.dual_seed_probes == c["dual_seed_probes"] > 0
    assert c["dual_skip_reads"] > 0 and c["dual_rewinds"] > 0
    ctx.close()
