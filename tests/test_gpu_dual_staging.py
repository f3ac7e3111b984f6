"""How the dual kernel (pgrc_amd/csrc/dualkern.h) brings a wave's next reads: a wave reserves a chunk of reads from the
work counter, stages 16 (or 32) of them at a time in LDS and hands them to the lanes that have finished; a lane leaves
when its wave's stage and chunk are used up and the counter is past the end of the set.  The texts are small, so a wave
reserves 64 reads per visit to the work counter and chunk and stage boundaries are met all the time.  Results must equal
the oracle's and those of the two ordinary passes (PGRC_DUAL=0); `dual["searched"]` must equal the number of reads the
kernel had to take, so none is lost and none taken twice."""
import functools

import numpy as np
import pytest

import oracle as orc
from util import assert_same_results, make_inputs

pytestmark = pytest.mark.gpu

N = ord("N")
SEED = {32: 24, 100: 38, 150: 38, 250: 38}           # the seed length per read length (NW 2, 7, 10, 16)
KMAX = 4
COUNTS = [1, 15, 16, 17, 63, 64, 65, 64 * 37 + 1]


@functools.lru_cache(maxsize=None)
def inputs(L):
    """one text and the longest read set per read length; every case takes a prefix of the reads"""
    pg, reads = make_inputs(200_000, 64 * 37 + 1, L, seed=700 + L, pool_div=32)
    pg.setflags(write=False)
    reads.setflags(write=False)
    return pg, reads


@functools.lru_cache(maxsize=None)
def oracle_of_all(L):
    """the oracle's result for the whole read set of inputs(L), computed once: a read's result does not depend on the others"""
    pg, reads = inputs(L)
    o = orc.oracle_match("c", pg, reads, SEED[L], KMAX, 0)
    for a in o.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return o


def prefix(o, n):
    mism = o["mism"][:n]
    return {"pos": o["pos"][:n], "rc": o["rc"][:n], "mism": mism, "hist": np.bincount(mism, minlength=256).astype(o["hist"].dtype),
            "matched": int((mism != 255).sum())}


def run(monkeypatch, pg, reads, seed_len, dual, state=None):
    from pgrc_amd import MatchContext
    monkeypatch.setenv("PGRC_DUAL", dual)
    ctx = MatchContext(reads.shape[1], seed_len, KMAX, 0, "c")
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


def check(monkeypatch, pg, reads, seed_len, eligible, state=None, what="", o=None):
    """eligible: how many reads the dual kernel itself has to search; o: the oracle's result where it is known already"""
    if o is None:
        o = orc.oracle_match("c", pg, reads, seed_len, KMAX, 0, state=state)
    on, c_on = run(monkeypatch, pg, reads, seed_len, "1", state)
    off, c_off = run(monkeypatch, pg, reads, seed_len, "0", state)
    assert c_on["screened"] == 2, "the dual kernel did not run"
    assert c_off["screened"] != 2
    assert_same_results(on, o, f"{what}: dual kernel vs oracle")
    assert_same_results(off, o, f"{what}: two passes vs oracle")
    assert on["matched"] == o["matched"]
    assert c_on["dual"]["searched"] == eligible, f"{what}: {c_on['dual']['searched']} reads searched, {eligible} eligible"
    return c_on


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("L", [32, 100, 150, 250])
def test_read_counts_and_lengths(monkeypatch, L, n):
    """a partial last stage, a last chunk of one read, one wave / several waves; NW 7: a stage's 112 words are no multiple
    of 64; NW 16: stages of 32 reads"""
    pg, reads = inputs(L)
    whole = oracle_of_all(L)
    if n == reads.shape[0]:
        assert np.array_equal(prefix(whole, n)["hist"], whole["hist"]) and prefix(whole, n)["matched"] == whole["matched"]
    check(monkeypatch, pg, reads[:n], SEED[L], n, what=f"L {L}, {n} reads", o=prefix(whole, n))


def skip_runs(n):
    """runs of reads to skip: 16 or more and 64 or more, one at the very start, one at the very end, some inside"""
    m = np.zeros(n, dtype=bool)
    for lo, k in ((0, 70), (100, 16), (130, 33), (300, 64), (500, 129), (n - 81, 81)):
        m[lo:lo + k] = True
    return m


@pytest.mark.parametrize("L", [100, 150, 250])
def test_runs_of_reads_that_are_already_exact(monkeypatch, L):
    """reads that an earlier phase matched exactly (mism == 0 in the state handed in) are passed over: whole stages of
    them, at the start and at the end of the set"""
    pg, reads = inputs(L)
    n = 64 * 20 + 1
    reads = reads[:n].copy()
    rng = np.random.default_rng(L)
    skip = skip_runs(n)
    starts = rng.integers(0, pg.size - L, size=n)
    for i in np.flatnonzero(skip):
        reads[i] = pg[starts[i]:starts[i] + L]                       # (an exact forward alignment exists)
    first = orc.oracle_match("c", pg, reads, SEED[L], 2, 0, rev_compl=False)
    assert (first["mism"][skip] == 0).all()
    state = (first["pos"], first["rc"], first["mism"])
    eligible = int((first["mism"] != 0).sum())
    assert 0 < eligible <= n - int(skip.sum())
    check(monkeypatch, pg, reads, SEED[L], eligible, state=state, what=f"L {L}, exact runs")


@pytest.mark.parametrize("L", [100, 150, 250])
def test_runs_of_reads_with_many_ns(monkeypatch, L):
    """reads with more than four N go the byte path (N flag 1): the dual kernel passes them over; reads with 1-4 N,
    scattered among plain reads, are its own (their flag and N positions travel through the stage)"""
    pg, reads = inputs(L)
    n = 64 * 20 + 1
    reads = reads[:n].copy()
    rng = np.random.default_rng(1000 + L)
    skip = skip_runs(n)
    for i in np.flatnonzero(skip):
        reads[i, rng.choice(L, size=5 + int(rng.integers(0, 4)), replace=False)] = N
    few = np.flatnonzero(~skip)[::5]
    for t, i in enumerate(few):
        reads[i, rng.choice(L, size=1 + t % 4, replace=False)] = N
    c = check(monkeypatch, pg, reads, SEED[L], n - int(skip.sum()), what=f"L {L}, N runs")
    assert c["dual"]["searched"] > few.size


def test_reads_with_few_ns_in_every_stage(monkeypatch):
    """1-4 N in every third read of a set that ends one read into a chunk"""
    L = 150
    pg, reads = inputs(L)
    n = 64 * 9 + 1
    reads = reads[:n].copy()
    rng = np.random.default_rng(77)
    for t, i in enumerate(range(0, n, 3)):
        reads[i, rng.choice(L, size=1 + t % 4, replace=False)] = N
    check(monkeypatch, pg, reads, SEED[L], n, what="few N")
