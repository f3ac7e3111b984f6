"""The position array of the order-preserving paired mode (orgIdx2PgPos; pgrc_rlist_pair_positions): tests/rlist_util's numpy
restatement against its copy of the reference's loops, on seeded settings that include empty LQ / N lists, absent lists, T = 2
and positions on both sides of 2^32.  No GPU."""
import numpy as np

import rlist_util as rl


def test_numpy_form_equals_the_literal_loops_on_random_settings():
    seen = {"empty_lq": 0, "absent": 0, "T2": 0, "below": 0, "above": 0, "matched": 0}
    for seed in range(400):
        s = rl.make_setting(seed)
        assert (rl.writers_per_index(s["T"], s["hq"], s["lq"], s["n"], s["read_org"], s["match_pos"]) == 1).all()
        want = rl.positions_of(s, rl.positions_literal)
        got = rl.positions_of(s, rl.positions_numpy)
        assert got.dtype == np.uint64 and np.array_equal(got, want), seed
        assert (want != rl.FILL).all()
        seen["empty_lq"] += s["lq"] is not None and s["lq"][1].size == 0
        seen["absent"] += s["lq"] is None
        seen["T2"] += s["T"] == 2
        seen["below"] += bool((want < 2**32).any())
        seen["above"] += bool((want >= 2**32).any())
        seen["matched"] += bool((s["match_pos"] != rl.FILL).any())
    assert min(seen.values()) > 10, seen


def test_the_smallest_settings():
    for T in (2,):
        for seed in range(30):
            s = rl.make_setting(1000 + seed, T=T)
            assert np.array_equal(rl.positions_of(s, rl.positions_numpy), rl.positions_of(s, rl.positions_literal))
    # one list alone: the inclusive sums of off at the permuted indexes
    off, org = np.array([5, 0, 7, 65535], np.uint16), np.array([2, 0, 3, 1], np.uint32)
    want = np.array([5, 65547, 5, 12], np.uint64)
    for fn in (rl.positions_literal, rl.positions_numpy):
        assert np.array_equal(fn(4, (off, org), None, None, 0, 0), want)
    # bases: the LQ list starts at hq_len, the N list at hq_len + lq_len, above 2^32
    hq, lq, nn = (np.array([1], np.uint16), np.array([3], np.uint32)), (np.array([2, 2], np.uint16), np.array([0, 1], np.uint32)), (np.array([9], np.uint16), np.array([2], np.uint32))
    want = np.array([2**32 + 2, 2**32 + 4, 2**32 + 50 + 9, 1], np.uint64)
    for fn in (rl.positions_literal, rl.positions_numpy):
        assert np.array_equal(fn(4, hq, lq, nn, 2**32, 50), want)


def test_writers_per_index_finds_what_the_device_refuses():
    s = rl.make_setting(77, T=200)
    w = rl.writers_per_index(s["T"], s["hq"], s["lq"], s["n"], s["read_org"], s["match_pos"])
    assert (w == 1).all()
    off, org = s["hq"]
    if org.size < 2:
        off, org = np.zeros(2, np.uint16), np.array([0, 1], np.uint32)
    twice = org.copy()
    twice[0] = twice[1]
    w = rl.writers_per_index(s["T"], (off, twice), None, None)
    assert w.max() == 2
    # an unmatched read writes nothing, a matched one does
    mp = np.array([rl.NOT_MATCHED, 17], np.uint64)
    arr = rl.positions_literal(2, (np.array([4], np.uint16), np.array([0], np.uint32)), None, None, 0, 0, np.array([0, 1], np.uint32), mp)
    assert arr.tolist() == [4, 17]
