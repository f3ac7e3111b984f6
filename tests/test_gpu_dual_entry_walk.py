"""The dual kernel's walk over the entries a lane has at hand (pgrc_amd/csrc/dualkern.h): a lane goes over the entries
its iteration's load brought -- a head's one or two, a fetch from ent[] -- rejecting by the position test and the
fingerprint until one passes; that one goes on to the verify cache and the text.  The texts here carry planted repeat
families, so that buckets of 2 .. 13 entries and over-full ones are opened all the time, with fingerprint rejects and
passes at the first entry, at the last, and behind five rejects.

What makes the fingerprint reject: the sparsified hash of a K = 28 window ignores the eleven symbols IGN; they are the
entry's fingerprint, and an entry is rejected when more of them differ from the read's window than the limit in force
allows -- three differing symbols never reject under the starting limit of -M 50, so copies that differ by 0 - 3
substitutions alone would leave the fingerprint nothing to reject at a read's first seeds.  So a family has NEAR copies
(at most three substitutions against the family's base, none at a hashed symbol of the first window) and FAR copies (eight
of the eleven ignored symbols of the copy's first window substituted: the same bucket, a fingerprint more than three away
from every near copy).  Reads start at a copy's first symbol with a clean first window; some are reverse-complemented, the
last of a case carry 1 - 4 N.

The guard (at least 200 reads open a bucket of five or more entries, at least 50 meet a fingerprint pass behind a reject)
is worked out on the CPU from the oracle's index export, for the first seed of the 305 plain reads that every case of a
read length takes its reads from: the forward bucket of seed 0 is opened whatever happens later.

Every case is held to the oracle's dual query, to the compiled reference where it is present, and -- in its work
counters -- to the counters the parent commit's kernel gave on the same inputs (tests/golden/dual_entry_walk_counters.json,
recorded once with that build): the walk changes in which iteration an entry is looked at, not which entries are."""
import functools
import json
import os

import numpy as np
import pytest

import oracle as orc
from util import assert_same_results, revcomp

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dual_entry_walk_counters.json")
SEED_LEN = 38
K = 28
IGN = (3, 7, 11, 14, 15, 18, 19, 22, 23, 26, 27)    # window symbols the sparsified hash ignores (Hashes.h:54-76): the fingerprint
FAMILIES = (2, 3, 4, 5, 7, 8, 9, 13, 14, 20)         # copies per family: the two-entry head, one .. several fetches, the cap of 13, over-full
REPS = 3                                             # families per size, one per layout
G = 400_000
SLOT = 200                                           # copies start at multiples of it (and of the index's sampling step)
COUNTS = (1, 63, 64, 65, 64 * 5 + 1)
N_FULL = COUNTS[-1]
N_WITH_N = 16
GEN_SEED = {100: 4100, 150: 4150}
EQUAL = ("dual.candidates", "dual.verifies", "redo_reads", "dual_seed_probes", "dual_skip_reads", "dual_rewinds")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _substitute(rng, seq, offsets):
    for o in offsets:
        seq[o] = rng.choice(ACGT[ACGT != seq[o]])


def _layout(rep, f):
    """which copies of a family, in text order, are far ones"""
    if rep == 0:
        return [False] * f                                           # every entry passes
    if rep == 1:
        return [i < min(5, f - 1) for i in range(f)]                 # up to five rejects, then passes
    return [i % 3 != 0 for i in range(f)]                            # near, far, far, near, ...: passes at the first and in mid-walk


@functools.lru_cache(maxsize=None)
def inputs(L):
    """the text, the plain reads (shuffled: every case takes a prefix) and the reads with N of one read length"""
    rng = np.random.default_rng(GEN_SEED[L])
    pg = ACGT[rng.integers(0, 4, size=G)]
    slots = rng.permutation(G // SLOT - 2)
    used = 0
    big, small = [], []                                              # where the copies of families of five and more start, and of the others
    near_at = np.concatenate([np.array(IGN), np.arange(K, L)])       # (a near copy keeps the hashed symbols of its first window: the same bucket)
    for f in FAMILIES:
        for rep in range(REPS):
            base = ACGT[rng.integers(0, 4, size=L)]
            starts = np.sort(slots[used:used + f]) * SLOT
            used += f
            for p, far in zip(starts, _layout(rep, f)):
                c = base.copy()
                if far:
                    _substitute(rng, c, rng.choice(IGN, size=8, replace=False))
                else:
                    _substitute(rng, c, rng.choice(near_at, size=int(rng.integers(0, 4)), replace=False))
                pg[p:p + L] = c
                (big if f >= 5 else small).append(int(p))

    def read_at(p, n_sub, n_n=0):
        r = pg[p:p + L].copy()
        at = K + rng.choice(L - K, size=n_sub + n_n, replace=False)  # (the first window stays clean)
        _substitute(rng, r, at[:n_sub])
        r[at[n_sub:]] = ord("N")
        return r

    plain = [read_at(p, int(rng.integers(0, 3))) for p in big + small]
    plain += [revcomp(read_at(p, int(rng.integers(0, 3)))) for p in rng.choice(big + small, size=40, replace=False)]
    plain += [read_at(int(p), 1) for p in rng.integers(0, G - L, size=N_FULL - N_WITH_N - len(plain))]
    assert len(plain) == N_FULL - N_WITH_N
    plain = np.stack(plain)[rng.permutation(len(plain))]
    with_n = np.stack([read_at(p, t % 2, 1 + t % 4) if t % 3 else revcomp(read_at(p, t % 2, 1 + t % 4))
                       for t, p in enumerate(rng.choice(big, size=N_WITH_N, replace=False))])
    for a in (pg, plain, with_n):
        a.setflags(write=False)
    return pg, plain, with_n


def case_reads(L, n):
    """n reads: plain ones, then (as in the encoder's sum set) the reads with N"""
    _, plain, with_n = inputs(L)
    n_n = min(N_WITH_N, n // 20)
    return np.concatenate([plain[:n - n_n], with_n[:n_n]]), n_n


@functools.lru_cache(maxsize=None)
def guard(L):
    """From the oracle's index export alone, for the first seed of every plain read of the full set (the forward bucket of
    seed 0 is always opened, under the starting limit L // 50): how many reads open a bucket of five or more entries, and
    how many meet an entry the fingerprint lets through behind one it rejected."""
    pg, plain, _ = inputs(L)
    prm, cumm, positions = orc.oracle_index(pg, SEED_LEN)
    assert prm["K"] == K and SLOT % prm["k1"] == 0
    mask = prm["hash_size"] - 1
    kmax = L // 50
    ign = np.array(IGN)
    long_buckets = pass_behind_reject = 0
    for r in plain:
        h = orc.oracle().pgrc_or_copmem_hash(K, r[:K].tobytes()) & mask
        ents = np.sort(positions[int(cumm[h]):int(cumm[h + 1])])[:13]
        long_buckets += ents.size >= 5
        rejected = False
        for p in ents:
            p = int(p)
            if p + L > G:
                continue
            if int((pg[p + ign] != r[ign]).sum()) > kmax:
                rejected = True
            else:
                pass_behind_reject += rejected
                break
    return int(long_buckets), int(pass_behind_reject)


@functools.lru_cache(maxsize=None)
def expected(L, M):
    """the oracle's dual query (and the compiled reference) on all plain reads and all reads with N, computed once: a read's
    result does not depend on the others"""
    pg, plain, with_n = inputs(L)
    out = []
    for reads in (plain, with_n):
        o = orc.oracle_match_dual(pg, reads, SEED_LEN, L // M)
        if orc.have_ref():
            r = orc.ref_match("c", pg, reads, SEED_LEN, L // M, 0, n_nset=reads.shape[0] if reads is with_n else 0)
            for k in ("pos", "rc", "mism"):
                assert np.array_equal(o[k], r[k]), f"oracle and reference disagree on {k}"
        out.append(o)
    return out


def expected_for(L, M, n):
    (op, on), n_n = expected(L, M), min(N_WITH_N, n // 20)
    o = {k: np.concatenate([op[k][:n - n_n], on[k][:n_n]]) for k in ("pos", "rc", "mism")}
    o["hist"] = np.bincount(o["mism"], minlength=256).astype(op["hist"].dtype)
    o["matched"] = int((o["mism"] != 255).sum())
    return o


def run_case(L, M, skip, n):
    """the device's results and counters of one case (the caller has set PGRC_DUAL and PGRC_ROUND_SKIP)"""
    from pgrc_amd import MatchContext
    pg = inputs(L)[0]
    reads, _ = case_reads(L, n)
    ctx = MatchContext(L, SEED_LEN, L // M, 0, "c")
    ctx.set_pg_ascii(pg)
    ctx.set_reads_ascii(reads)
    ctx.set_profiling(True)
    ctx.init_results()
    ctx.run(True)
    pos, rc, mism, hist, matched = ctx.get_results()
    c = ctx.counters()
    ctx.close()
    assert c["screened"] == 2, "the dual kernel did not run"
    flat = {"dual." + k: int(v) for k, v in c["dual"].items()}
    flat.update({k: int(c[k]) for k in ("redo_reads", "dual_seed_probes", "dual_skip_reads", "dual_rewinds")})
    return {"pos": pos, "rc": rc, "mism": mism, "hist": hist, "matched": matched}, flat


def case_id(L, M, skip, n):
    return f"L{L}-M{M}-skip{skip}-n{n}"


def set_env(monkeypatch, skip):
    monkeypatch.setenv("PGRC_DUAL", "1")
    monkeypatch.setenv("PGRC_ROUND_SKIP", str(skip))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("skip", [1, 0])
@pytest.mark.parametrize("M", [50, 3])
@pytest.mark.parametrize("L", [100, 150])
def test_entry_walk(monkeypatch, L, M, skip, n):
    """-M 50: limits of 2 or 3, where the fingerprint rejects from the first seed on; -M 3: limits of 33 or 50, where the
    falses budget, the redo in the reference's order and the truncation to four entries come into play"""
    long_buckets, pass_behind_reject = guard(L)
    assert long_buckets >= 200, f"only {long_buckets} reads open a bucket of five or more entries"
    assert pass_behind_reject >= 50, f"only {pass_behind_reject} reads meet a fingerprint pass behind a reject"
    set_env(monkeypatch, skip)
    got, c = run_case(L, M, skip, n)
    assert_same_results(got, expected_for(L, M, n), case_id(L, M, skip, n))
    with open(GOLDEN) as f:
        parent = json.load(f)[case_id(L, M, skip, n)]
    for k in EQUAL:
        assert c[k] == parent[k], f"{k}: {c[k]}, the parent's kernel {parent[k]}"
    assert c["dual.entry_fetches"] <= parent["dual.entry_fetches"]
    assert c["dual.searched"] == n
