"""The divided read sets on the device (include/pgrc_readsets.h, pgrc_amd.DividedReadsSets) against the reference's loops
restated line by line (tests/rsets_util.py) and the fixtures of the compiled reference (tests/golden/rsets_*.npz): rows,
mappings with their guard and counts byte for byte, every refusal followed by a good call on the same object, and the chain
divider -> sets -> overlap search -> move -> matcher -> removal without a row crossing the link."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import rsets_util as ru

pytestmark = pytest.mark.gpu

E_PARAM, E_STATE = 1, 6
LS = (1, 21, 100, 150, 255)                 # row bytes 1, 6 / 7, 25 / 34, 38 / 50, 64 / 85
COUNTS = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193)
DENSITIES = (0.0, 1.0, 0.5, "one")
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ru.GOLDEN, "rsets_*.npz")))


def make_sets(st, L, separate_n, batches=1):
    from pgrc_amd import DividedReadsSets
    s = DividedReadsSets(L, separate_n, False)
    if batches == 1:
        s.append(ru.state_batch(st, L, separate_n))
    else:                                   # three batches, the middle one empty
        cut = st["A"] // 3
        for b, n in ru.split_batches(st, L, separate_n, [0, cut, cut, st["A"]]):
            s.append(b, n)
    s.finish()
    return s


def make_flags(rng, n, density):
    if density == "one":
        f = np.zeros(n, np.uint8)
        if n:
            f[rng.integers(n)] = 1
        return f
    return (rng.random(n) < density).astype(np.uint8)


def on_device(flags):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(flags)).cuda()
    torch.cuda.synchronize()
    return t, (t.data_ptr() if flags.size else 0)


def check(sets, want, what):
    got = ru.device_state(sets)
    i = sets.info()
    assert i["reads_total_count"] == want["A"], what
    assert i["count"][0] == want["hq"].shape[0] and i["count"][1] == want["lq"].shape[0], what
    assert ru.same_state(got, want), what


def edit_sequence(st, L, separate_n, rng, density, batches, device_flags):
    """move, move again, the HQ mapping, remove: each against the literal loops"""
    s = make_sets(st, L, separate_n, batches)
    check(s, st, "as appended")
    cur = st
    for step, d in enumerate((density, 0.5)):
        f = make_flags(rng, cur["hq"].shape[0], d)
        if device_flags:
            keep, p = on_device(f)
            s.move_lq(p, on_device=True)
        else:
            s.move_lq(f)
        cur = ru.literal_move(cur, f)
        check(s, cur, f"move {step}")
    assert np.array_equal(s.get_mapping("hq"), ru.literal_hq_mapping(cur))
    g = make_flags(rng, cur["lq"].shape[0] + (cur["n"].shape[0] if separate_n else 0), density)
    if device_flags:
        keep, p = on_device(g)
        s.remove(p, on_device=True)
    else:
        s.remove(g)
    cur = ru.literal_remove(cur, g)
    check(s, cur, "remove")
    assert np.array_equal(s.get_mapping("hq"), ru.literal_hq_mapping(cur))
    t = s.timing()
    assert t["edit"] == 3
    s.close()


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("k", range(len(COUNTS)))
def test_edits_equal_the_literal_loops(L, k):
    counts = (COUNTS[k], COUNTS[(k + 5) % len(COUNTS)], COUNTS[(k + 7) % len(COUNTS)])
    separate_n = (k + L) % 2 == 0
    rng = np.random.default_rng(1000 * L + k)
    st = ru.state_with_counts(rng, L, separate_n, counts)
    for j, density in enumerate(DENSITIES):
        edit_sequence(st, L, separate_n, rng, density, batches=1 if (j + k) % 2 else 3, device_flags=(j + k // 2) % 2 == 0)


def test_edits_of_300k_rows_per_set():
    rng = np.random.default_rng(5)
    st = ru.state_with_counts(rng, 150, True, (300000, 300000, 300000))
    s = make_sets(st, 150, True, 3)
    f = make_flags(rng, 300000, 0.5)
    s.move_lq(f)
    cur = ru.literal_move(st, f)
    check(s, cur, "move")
    t = s.timing()
    assert t["edit"] == 1 and t["rows_moved"] == 600000 and t["bytes_moved"] == 600000 * 38
    g = make_flags(rng, cur["lq"].shape[0] + 300000, 0.5)
    keep, p = on_device(g)
    s.remove(p, on_device=True)
    check(s, ru.literal_remove(cur, g), "remove")
    s.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_of_the_compiled_reference(name):
    assert len(FIXTURES) >= 8
    fx = ru.load_fixture(name)
    s = make_sets(fx["before"], fx["L"], fx["separate_n"])
    check(s, fx["before"], "before")
    s.move_lq(fx["is_hq"])
    check(s, fx["moved"], "moved")
    assert np.array_equal(s.get_mapping("hq"), fx["hq_mapping"])
    s.remove(fx["is_mapped"])
    check(s, fx["removed"], "removed")
    s.close()


def _code(fn, *a, **k):
    from pgrc_amd import PgrcMatchError
    try:
        fn(*a, **k)
    except PgrcMatchError as e:
        return e.code
    return 0


def test_refusals_leave_the_object_usable():
    from pgrc_amd import DividedReadsSets, MatchContext, OverlapFinder, _lib
    lib = _lib.lib
    L, sep = 21, True
    rng = np.random.default_rng(9)
    st = ru.state_with_counts(rng, L, sep, (40, 30, 20))
    good = ru.state_batch(st, L, sep)
    s = DividedReadsSets(L, sep, False)
    h = s._h
    # wrong struct_size, NULL pointers
    prm = _lib.RsetsParams(4, L, 1, 0, -1)
    out = C.c_void_p()
    assert lib.pgrc_rsets_create(C.byref(prm), C.byref(out)) == E_PARAM and not out.value
    assert lib.pgrc_rsets_create(None, C.byref(out)) == E_PARAM
    assert lib.pgrc_rsets_append(h, None, 0) == E_PARAM
    info = _lib.RsetsInfo(8)
    assert lib.pgrc_rsets_get_info(h, C.byref(info)) == E_PARAM and lib.pgrc_rsets_get_info(h, None) == E_PARAM
    # edits and hand-overs before finish
    ovl = OverlapFinder()
    assert _code(s.move_lq, np.ones(1, np.uint8)) == E_STATE
    assert _code(s.remove, np.ones(1, np.uint8)) == E_STATE
    assert _code(s.get_mapping, "hq") == E_STATE and _code(s.get_mapping, "lq") == E_STATE
    assert _code(s.overlap, "hq", ovl) == E_STATE
    assert _code(s.move_by_overlap, ovl) == E_STATE
    matcher = MatchContext(100, 38, 3, 0, "c", device=0)
    assert _code(s.to_matcher, matcher) == E_STATE and _code(s.remove_matched, matcher) == E_STATE
    # refused batches: the object stays empty
    def bad(**kw):
        b = dict(good)
        n_records = kw.pop("n_records", None)
        b.update(kw)
        return _code(s.append, b, n_records)
    assert bad(lq_index=good["lq_index"][::-1].copy()) == E_PARAM                       # does not ascend
    twice = good["lq_index"].copy()
    twice[1] = twice[0]
    assert bad(lq_index=twice) == E_PARAM                                               # an entry twice
    high = good["lq_index"].copy()
    high[-1] = st["A"]
    assert bad(lq_index=high) == E_PARAM                                                # an index >= A
    both = np.sort(np.unique(np.concatenate([[good["lq_index"][3]], good["n_index"][1:]]))).astype(np.uint32)
    assert both.size == good["n_index"].size and bad(n_index=both) == E_PARAM           # an index in both mappings
    assert bad(n_records=st["A"] + 1) == E_PARAM                                        # HQ count != A - LQ - N
    assert bad(n_hq=2 ** 32 - 1 - 50, n_records=2 ** 32 - 1) == E_PARAM                 # A > 2^32 - 2
    assert lib.pgrc_rsets_get_rows(h, 3, 0, 0, None) == E_PARAM and lib.pgrc_rsets_dispose(h, 5) == E_PARAM
    assert s.info()["reads_total_count"] == 0 and s.info()["count"] == (0, 0, 0)
    # ... and takes the good batch
    s.append(good)
    s.finish()
    assert _code(s.append, good) == E_STATE                                             # append after finish
    check(s, st, "after the refusals")
    assert lib.pgrc_rsets_move_lq(h, None, 0) == E_PARAM and lib.pgrc_rsets_remove(h, None, 0) == E_PARAM
    assert lib.pgrc_rsets_get_mapping(h, 1, None) == E_PARAM and lib.pgrc_rsets_get_mapping(h, 7, None) == E_PARAM
    assert lib.pgrc_rsets_get_rows(h, 0, 39, 2, None) == E_PARAM                        # rows outside the set
    assert lib.pgrc_rsets_overlap(h, 0, None, 1.0, 1, None, None) == E_PARAM
    assert lib.pgrc_rsets_to_matcher(h, None) == E_PARAM and lib.pgrc_rsets_remove_matched(h, None) == E_PARAM
    assert _code(s.move_by_overlap, ovl) == E_STATE                                     # no run of pgrc_rsets_overlap on this set
    assert _code(s.to_matcher, matcher) == E_PARAM                                      # a matcher of another read length
    assert _code(s.remove_matched, matcher) == E_PARAM                                  # ... and without LQ + N reads
    matcher.close()
    t = _lib.RsetsTiming(C.sizeof(_lib.RsetsTiming))
    assert lib.pgrc_rsets_get_timing(h, C.byref(t)) == E_STATE
    check(s, st, "after more refusals")
    f = make_flags(rng, 40, 0.5)
    s.move_lq(f)
    cur = ru.literal_move(st, f)
    check(s, cur, "the good move")
    # an overlap run, then an edit: the run no longer describes the HQ set
    s.overlap("hq", ovl, 1.0)
    s.move_lq(np.ones(cur["hq"].shape[0], np.uint8))
    assert _code(s.move_by_overlap, ovl) == E_STATE
    check(s, cur, "a move of nothing")
    # disposed sets
    s.dispose("n")
    assert _code(s.remove, np.zeros(cur["lq"].shape[0] + 20, np.uint8)) == E_STATE
    assert _code(s.move_lq, np.ones(cur["hq"].shape[0], np.uint8)) == E_STATE
    assert _code(s.get_rows, "n") == E_STATE and _code(s.get_mapping, "hq") == E_STATE
    assert np.array_equal(s.get_rows("lq"), cur["lq"]) and np.array_equal(s.get_mapping("lq"), cur["lq_map"])
    s.dispose("hq")
    assert _code(s.overlap, "hq", ovl) == E_STATE and s.info()["disposed"] == (True, False, True)
    s.close()
    ovl.close()
    # a move with n_reads_lq set: the alphabets differ
    q = DividedReadsSets(L, False, True)
    assert q.info()["symbols"] == (4, 5, 0) and q.info()["row_bytes"] == (6, 7, 0)
    q.append({"n_hq": 3, "n_lq": 1, "n_n": 0, "symbols": (4, 5, 0), "row_bytes": (6, 7, 0), "hq_rows": np.zeros((3, 6), np.uint8),
              "lq_rows": np.zeros((1, 7), np.uint8), "n_rows": np.zeros(0, np.uint8), "lq_index": np.array([2], np.uint32),
              "n_index": np.zeros(0, np.uint32)})
    q.finish()
    assert _code(q.move_lq, np.zeros(3, np.uint8)) == E_PARAM
    q.remove(np.array([1], np.uint8))
    assert q.info()["count"] == (3, 0, 0) and np.array_equal(q.get_mapping("lq"), [4]) and np.array_equal(q.get_mapping("hq"), [0, 1, 2, 3, 4])
    q.close()


def test_a_move_after_a_removal_is_refused():
    """the removed reads are in neither mapping and not in the HQ set: a move's flags, one per HQ row, do not cover them"""
    from pgrc_amd import OverlapFinder
    L, sep = 21, True
    rng = np.random.default_rng(17)
    st = ru.state_with_counts(rng, L, sep, (300, 200, 100))
    s = make_sets(st, L, sep)
    ovl = OverlapFinder()
    s.overlap("hq", ovl, 1.0)
    g = make_flags(rng, 300, 0.5)
    assert 0 < int(g.sum()) < 300
    s.remove(g)
    cur = ru.literal_remove(st, g)
    check(s, cur, "remove")
    flags = make_flags(rng, 300, 0.5)
    keep, p = on_device(flags)
    assert _code(s.move_lq, flags) == E_PARAM and _code(s.move_lq, p, on_device=True) == E_PARAM
    assert _code(s.move_by_overlap, ovl) == E_PARAM                 # (the run still describes the HQ set: it is the counts that refuse)
    check(s, cur, "after the refused moves")
    assert np.array_equal(s.get_mapping("hq"), ru.literal_hq_mapping(cur))
    g2 = make_flags(rng, cur["lq"].shape[0] + cur["n"].shape[0], 0.5)
    s.remove(g2)
    check(s, ru.literal_remove(cur, g2), "a second removal")
    s.close()
    ovl.close()


# ------------------------------------------------------------------------------------------------ the chain
def chain_records(seed=11, n=20000, L=100, coverage=20):
    """reads of a random genome at the given coverage; every 40th read holds an N, every 4th of the others is of low quality
    under the simplified suffix rule at error limit 0.05, every 5th is noisy"""
    rng = np.random.default_rng(seed)
    G = n * L // coverage
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=G)]
    start = rng.integers(0, G - L, size=n)
    reads = genome[start[:, None] + np.arange(L)[None, :]].copy()
    with_n = np.arange(n) % 40 == 7
    reads[with_n, rng.integers(0, L, size=int(with_n.sum()))] = ord("N")
    quals = np.full((n, L), ord("I"), np.uint8)
    low = (np.arange(n) % 4 == 1) & ~with_n
    quals[low, int(L * (1 - 0.05))] = ord("#")
    noisy = np.flatnonzero(np.arange(n) % 5 == 3)               # reads that neither overlap nor map: 12 symbols drawn anew
    for r in noisy:
        at = rng.choice(L, size=12, replace=False)
        reads[r, at] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=12)]
    return genome, reads, quals


def test_chain_without_a_row_crossing_the_link():
    from pgrc_amd import DividedPCLReadsSets, DividedReadsSets, MatchContext, OverlapFinder, NOT_MATCHED_POS
    L = 100
    genome, reads, quals = chain_records(L=L)
    div = DividedPCLReadsSets(L, 0.05, True, True, False)
    batch = div.divide(reads, quals)
    assert batch["n_hq"] > 10000 and batch["n_lq"] > 3000 and batch["n_n"] > 300
    a = DividedReadsSets(L, True, False)
    a.append_divider(div)
    a.finish()
    b = DividedReadsSets(L, True, False)
    b.append(batch)
    b.finish()
    st = ru.device_state(b)
    assert ru.same_state(ru.device_state(a), st)
    assert np.array_equal(st["hq"].ravel(), batch["hq_rows"]) and np.array_equal(st["lq_map"][:-1], batch["lq_index"]) and st["lq_map"][-1] == 20000
    assert np.array_equal(st["n"].ravel(), batch["n_rows"]) and np.array_equal(st["n_map"][:-1], batch["n_index"])
    # the overlap search on the set's rows where they lie, under both rules
    for rule in ("parallel", "serial"):
        host, dev = OverlapFinder(), OverlapFinder()
        want = host.run(st["hq"], L, 4, 0.6, rule=rule)
        dev.set_rule(rule)
        got = a.overlap("hq", dev, 0.6)
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), (rule, k)
        flags = host.both_sides()
        assert np.array_equal(dev.both_sides(), flags) and dev.rule_info() == host.rule_info()
        assert dev.timing()["bytes_up"] == 0 and host.timing()["bytes_up"] == st["hq"].size
        host.close()
        if rule == "parallel":
            dev.close()
    assert 0 < int(flags.sum()) < flags.size
    a.move_by_overlap(dev)
    b.move_lq(flags)
    moved = ru.literal_move(st, flags)
    assert ru.same_state(ru.device_state(a), moved) and ru.same_state(ru.device_state(b), moved)
    assert np.array_equal(a.get_mapping("hq"), ru.literal_hq_mapping(moved))
    dev.close()
    # the LQ + N sum set to the matcher on the device, and by the host route
    nl, nn = moved["lq"].shape[0], moved["n"].shape[0]
    res = []
    ctxs = []
    for route in ("device", "host"):
        ctx = MatchContext(L, 38, 3, 0, "c", device=0)
        ctx.set_pg_ascii(genome)
        if route == "device":
            a.to_matcher(ctx)
            assert ctx.n == nl + nn
        else:
            ctx.set_reads_packed_sets([(moved["lq"], nl, 4), (moved["n"], nn, 5)])
        ctx.init_results()
        ctx.run(True)
        res.append(ctx.get_results())
        ctxs.append(ctx)
    for x, y in zip(res[0][:4], res[1][:4]):
        assert np.array_equal(x, y)
    assert res[0][4] == res[1][4] and 0 < res[0][4] < nl + nn
    a.remove_matched(ctxs[0])
    mapped = (res[1][0] != np.uint64(NOT_MATCHED_POS)).astype(np.uint8)
    b.remove(mapped)
    removed = ru.literal_remove(moved, mapped)
    assert ru.same_state(ru.device_state(a), removed) and ru.same_state(ru.device_state(b), removed)
    assert np.array_equal(a.get_mapping("hq"), ru.literal_hq_mapping(removed))
    for c in ctxs:
        c.close()
    for x in (a, b, div):
        x.close()
