"""The dual kernel's packed result (pgrc_amd/csrc/dualkern.h, "The packed result"; k_unpack_results in results.hip): a
finished read is one 8-byte store of position | count << 40 | strand << 48 | tag, and a streaming pass right behind the
kernel takes the tagged words apart.  Every case holds pos, rc, mism, the histogram and the matched count to the oracle,
and byte for byte to the SAME context under PGRC_DUAL_PACK=0 (three stores per read, no pass), whose work counters
must be the same too: small read sets around the wave size, reads that come with an earlier result, reads with N on both
of their paths within one wave, the streamed hand-over and a sharded context."""
import numpy as np
import pytest

import oracle as orc
from util import assert_same_results, make_inputs, pack_rows, revcomp

pytestmark = pytest.mark.gpu

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
SEED_LEN = 38
G = 200_000
COUNTS = (1, 63, 64, 65, 64 * 37 + 1)
_cache = {}


def text():
    if "pg" not in _cache:
        _cache["pg"] = make_inputs(G, 1, 100, seed=4062, pool_div=32)[0]
    return _cache["pg"]


def reads_for(L, n, seed):
    """n reads of length L: text windows of both strands with 0-3 substitutions; every eighth read is random"""
    key = (L, n, seed)
    if key not in _cache:
        pg = text()
        rng = np.random.default_rng(seed)
        reads = rng.choice(_ACGT, size=(n, L))
        for i in range(n):
            if i % 8 == 7:
                continue
            st = int(rng.integers(0, pg.size - L))
            r = pg[st:st + L].copy()
            if rng.integers(0, 2):
                r = revcomp(r)
            for x in rng.choice(L, size=int(rng.integers(0, 4)), replace=False):
                r[x] = _ACGT[(np.flatnonzero(_ACGT == r[x])[0] + 1 + int(rng.integers(0, 3))) % 4]
            reads[i] = r
        _cache[key] = reads
    return _cache[key]


def results_of(ctx):
    pos, rc, mism, hist, matched = ctx.get_results()
    return {"pos": pos, "rc": rc, "mism": mism, "hist": hist, "matched": matched}


def work_of(ctx):
    c = ctx.counters()
    assert c["screened"] == 2, "the dual kernel did not run"
    return {"dual": {k: int(v) for k, v in c["dual"].items()}, "dual_seed_probes": int(c["dual_seed_probes"]), "redo_reads": int(c["redo_reads"])}


def run_both(monkeypatch, ctx, state=None):
    """the context's results and work counters with the packed store (the default) and with PGRC_DUAL_PACK=0"""
    out = []
    for pack in ("1", "0"):
        monkeypatch.setenv("PGRC_DUAL_PACK", pack)
        ctx.reload_options()
        if state is None:
            ctx.init_results()
        else:
            ctx.set_results(*state)
        ctx.run(True)
        out.append((results_of(ctx), work_of(ctx)))
    return out


def check(monkeypatch, ctx, o, what, state=None):
    (on, c_on), (off, c_off) = run_both(monkeypatch, ctx, state)
    assert on["pos"].max(initial=0) < (1 << 40) or (on["pos"][on["pos"] >= (1 << 40)] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), f"{what}: a packed word was left behind"
    assert_same_results(on, o, what + ", packed vs oracle")
    assert_same_results(off, o, what + ", three stores vs oracle")
    for k in ("pos", "rc", "mism"):
        assert on[k].tobytes() == off[k].tobytes(), f"{what}: {k} differs between PGRC_DUAL_PACK=1 and 0"
    assert c_on == c_off, f"{what}: work counters {c_on} with the packed store, {c_off} without"
    return on


def context(L, kmax, pg, reads, devices=None):
    from pgrc_amd import MatchContext
    ctx = MatchContext(L, SEED_LEN, kmax, 0, "c", devices=devices)
    ctx.set_pg_ascii(pg)
    ctx.set_reads_ascii(reads)
    ctx.set_profiling(True)
    return ctx


@pytest.mark.parametrize("pos64", [0, 1])
@pytest.mark.parametrize("M", [50, 3])
@pytest.mark.parametrize("L", [100, 150])
def test_small_read_sets(monkeypatch, L, M, pos64):
    """read counts around a wave and a stage (1, 63, 64, 65) and one of 37 waves and a read; -M 50: limits of 2 or 3,
    -M 3: limits of 33 or 50 (the redo in the reference's order); the 64-bit-position instances as well"""
    monkeypatch.setenv("PGRC_DUAL", "1")
    monkeypatch.setenv("PGRC_FORCE_POS64", str(pos64))
    pg = text()
    for n in COUNTS:
        reads = reads_for(L, n, seed=L + n)
        o = orc.oracle_match("c", pg, reads, SEED_LEN, L // M, 0)
        ctx = context(L, L // M, pg, reads)
        got = check(monkeypatch, ctx, o, f"L {L} -M {M} n {n} pos64 {pos64}")
        ctx.close()
        if n > 64:
            assert (got["rc"][got["mism"] != 255] == 1).any() and (got["rc"][got["mism"] != 255] == 0).any()
            assert (got["mism"] == 255).any() and (got["mism"] == 0).any() and ((got["mism"] > 0) & (got["mism"] < 255)).any()


@pytest.mark.parametrize("pos64", [0, 1])
def test_second_phase_keeps_what_it_does_not_improve(monkeypatch, pos64):
    """A third of the reads arrive with an earlier result (count 0 .. 3 -- below this run's limit of 5, as a phase with
    a lower limit leaves them -- any position, either strand flag).  The run improves some (a better alignment exists) and
    must leave the others' three values as they came, bit for bit: the pass stores nothing for a read without the tag."""
    monkeypatch.setenv("PGRC_DUAL", "1")
    monkeypatch.setenv("PGRC_FORCE_POS64", str(pos64))
    L, n, kmax = 150, 64 * 37 + 1, 5
    pg, reads = text(), reads_for(150, 64 * 37 + 1, seed=77)
    rng = np.random.default_rng(78)
    pos = np.full(n, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    rc = np.zeros(n, dtype=np.uint8)
    mism = np.full(n, 255, dtype=np.uint8)
    early = np.arange(0, n, 3)
    pos[early] = rng.integers(0, pg.size - L, size=early.size).astype(np.uint64)
    rc[early] = rng.integers(0, 2, size=early.size).astype(np.uint8)
    mism[early] = rng.integers(0, 4, size=early.size).astype(np.uint8)
    state = (pos, rc, mism)
    o = orc.oracle_match("c", pg, reads, SEED_LEN, kmax, 0, state=state)
    ctx = context(L, kmax, pg, reads)
    got = check(monkeypatch, ctx, o, f"second phase pos64 {pos64}", state=state)
    ctx.close()
    improved = got["mism"][early] < mism[early]
    assert improved.sum() >= 50 and (~improved).sum() >= 50, "the case must hold reads that are improved and reads that are not"
    kept = early[~improved]
    for k, before in (("pos", pos), ("rc", rc), ("mism", mism)):
        assert got[k][kept].tobytes() == before[kept].tobytes(), f"{k} of a read that was not improved changed"


def test_reads_with_n_on_both_paths_within_a_wave(monkeypatch):
    """Reads with 1-4 N are the dual kernel's own (packed store, unpacked); reads with more go the byte path, whose kernel
    stores beside the pass.  Both kinds and reads without N alternate, so every 64 consecutive reads hold all three.  (An N
    is a mismatch: a limit of 12 lets reads with 7 N and 3 substitutions match.)"""
    monkeypatch.setenv("PGRC_DUAL", "1")
    L, n, kmax = 150, 64 * 37 + 1, 12
    pg = text()
    reads = reads_for(L, n, seed=91).copy()
    rng = np.random.default_rng(92)
    for i in range(n):
        if i % 3 == 1:
            reads[i, rng.choice(L, size=1 + i % 4, replace=False)] = ord("N")
        elif i % 3 == 2:
            reads[i, rng.choice(L, size=5 + i % 3, replace=False)] = ord("N")
    o = orc.oracle_match("c", pg, reads, SEED_LEN, kmax, 0)
    ctx = context(L, kmax, pg, reads)
    got = check(monkeypatch, ctx, o, "reads with N")
    ctx.close()
    few, many = np.arange(1, n, 3), np.arange(2, n, 3)
    assert (got["mism"][few] != 255).sum() >= 100 and (got["mism"][many] != 255).sum() >= 100


@pytest.mark.parametrize("n_nset", [0, 200])
def test_streamed_hand_over(monkeypatch, n_nset):
    """three blocks, the middle one a single read; with reads holding N the last block is the N set.  A block's results
    are downloaded behind the event recorded after its kernel AND its pass."""
    from pgrc_amd import MatchContext
    monkeypatch.setenv("PGRC_DUAL", "1")
    L, n, kmax = 150, 64 * 37 + 1, 3
    pg = text()
    reads = reads_for(L, n, seed=55).copy()
    rng = np.random.default_rng(56)
    for i in range(n - n_nset, n):
        reads[i, rng.choice(L, size=1 + i % 6, replace=False)] = ord("N")
    o = orc.oracle_match("c", pg, reads, SEED_LEN, kmax, 0)
    ctx = context(L, kmax, pg, reads)
    resident = check(monkeypatch, ctx, o, f"resident run, {n_nset} reads with N")
    ctx.close()
    a = 1000
    if n_nset:
        sets = [(pack_rows(reads[:a]), a, 4), (pack_rows(reads[a:a + 1]), 1, 4), (pack_rows(reads[a + 1:n - n_nset]), n - n_nset - a - 1, 4),
                (pack_rows(reads[n - n_nset:], b"ACGNT"), n_nset, 5)]
    else:
        sets = [(pack_rows(reads[:a]), a, 4), (pack_rows(reads[a:a + 1]), 1, 4), (pack_rows(reads[a + 1:]), n - a - 1, 4)]
    for pack in ("1", "0"):
        monkeypatch.setenv("PGRC_DUAL_PACK", pack)
        st = MatchContext(L, SEED_LEN, kmax, 0, "c")
        st.set_pg_ascii(pg)
        st.prepare_index(True)
        pos, rc, mism, hist, matched = st.match_streamed(sets)
        got = {"pos": pos, "rc": rc, "mism": mism, "hist": hist, "matched": matched}
        assert_same_results(got, o, f"streamed, PGRC_DUAL_PACK={pack}")
        assert st.counters()["screened"] == 2
        for k in ("pos", "rc", "mism"):
            assert got[k].tobytes() == resident[k].tobytes(), f"streamed {k} differs from the resident run's"
        assert_same_results(results_of(st), o, f"streamed, what the device holds, PGRC_DUAL_PACK={pack}")
        st.close()


def test_three_shards(monkeypatch):
    monkeypatch.setenv("PGRC_DUAL", "1")
    L, n, kmax = 150, 64 * 37 + 1, 3
    pg = text()
    reads = reads_for(L, n, seed=55)
    o = orc.oracle_match("c", pg, reads, SEED_LEN, kmax, 0)
    out = []
    for pack in ("1", "0"):
        monkeypatch.setenv("PGRC_DUAL_PACK", pack)
        ctx = context(L, kmax, pg, reads, devices=[0, 0, 0])
        ctx.init_results()
        ctx.run(True)
        out.append(results_of(ctx))
        ctx.close()
        assert_same_results(out[-1], o, f"three shards, PGRC_DUAL_PACK={pack}")
    for k in ("pos", "rc", "mism"):
        assert out[0][k].tobytes() == out[1][k].tobytes()
