"""tests/listarchive_util's two restatements of the archive form of a reads list's mismatch streams -- the literal loops of the
reference's three encoder functions and of its loader, and the parallel form the device follows -- against every
reference-made fixture (tests/golden/listarchive_*.npz, make_golden_listarchive.py) in both directions, and against each other
on about 300 random generator settings.  No GPU."""
import json
import os

import numpy as np
import pytest

import decode_util as du
import listarchive_util as la

FIXTURES = la.fixtures()
NAMES = {"mixed", "ties", "no_mismatches", "fast", "max_one", "wide", "one_entry"}


def test_the_fixture_set_is_complete():
    assert {la.case_name(p) for p in FIXTURES} == NAMES
    m = json.load(open(os.path.join(la.GOLDEN, "manifest_listarchive.json")))
    assert set(m) == NAMES
    assert m["mixed"]["limit"] == 6 and m["mixed"]["dest_len"][4] == 0 and m["mixed"]["order"] != "ACGTN"
    assert m["wide"]["limit"] == 254 and m["fast"]["fast"] and m["max_one"]["limit"] == 1 and m["no_mismatches"]["limit"] == 0


@pytest.mark.parametrize("path", FIXTURES, ids=la.case_name)
@pytest.mark.parametrize("encode", [la.encode_literal, la.encode_parallel], ids=["literal", "parallel"])
def test_encoders_equal_the_reference(path, encode):
    L, fast, (cnt, sym, off, rev_off), st, _ = la.load_case(path)
    assert np.array_equal(rev_off, du.offsets_to_rev_offsets(cnt, off, L).astype(np.uint8))      # the builder's stream, two ways
    la.assert_streams(encode(cnt, sym, rev_off, fast), st)
    codes, order = du.exclusive_encoding(sym)           # the restatement the decoder's tests have used so far
    assert order == st["bases_order"] and np.array_equal(codes, st["mis_sym"])


@pytest.mark.parametrize("path", FIXTURES, ids=la.case_name)
@pytest.mark.parametrize("load", [la.load_literal, la.load_parallel], ids=["literal", "parallel"])
def test_loaders_equal_the_reference(path, load):
    L, _, (cnt, _, off, _), st, (lcnt, lsym, loff) = la.load_case(path)
    got = load(st, L)
    for g, w in zip(got, (lcnt, lsym, loff)):
        assert g.dtype == np.uint8 and g.tobytes() == w.tobytes()
    assert np.array_equal(got[0], cnt) and np.array_equal(got[2], off)


def _settings():
    rng = np.random.default_rng(20)
    for k in range(300):
        L = int(rng.choice([16, 100, 150, 255]))
        hi = int(rng.choice([1, 3, 6, min(L, 40), min(L, 254)]))
        counts = sorted(set(int(x) for x in rng.integers(1, hi + 1, size=int(rng.integers(1, 6)))))
        yield dict(seed=1000 + k, n=int(rng.choice([0, 1, 2, 65, 300, 1500])), L=L, zero=float(rng.choice([0.0, 0.5, 0.95, 1.0])), counts=tuple(counts),
                   skew=tuple(float(x) for x in rng.integers(0, 4, size=5) + (rng.random(5) < 0.3)), same=float(rng.choice([0.0, 0.1]))), bool(k % 3 == 0)


def test_literal_and_parallel_forms_agree_on_random_settings():
    seen_limits = set()
    for knobs, fast in _settings():
        if not sum(knobs["skew"]):
            knobs["skew"] = (1, 1, 1, 1, 1)
        cnt, sym, rev_off = la.make_list(**knobs)
        lit = la.encode_literal(cnt, sym, rev_off, fast)
        la.assert_streams(la.encode_parallel(cnt, sym, rev_off, fast), lit)
        seen_limits.add(int(lit["props"][0]))
        a, b = la.load_literal(lit, knobs["L"]), la.load_parallel(lit, knobs["L"])
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), knobs
        assert np.array_equal(a[0], cnt) and np.array_equal(a[2], du.rev_offsets_to_offsets(cnt, rev_off, knobs["L"]).astype(np.uint8))
    assert {0, 1}.issubset(seen_limits) and max(seen_limits) > 100
