"""The checker of the overlap search under the rule of the parallel generator against the reference, without a GPU:
tests/pgovl_par_util's literal loops and its array form give what the compiled reference gave, at 1 and at 8 threads, for every
fixture of tests/golden/make_golden_pgovl_par.py -- nextRead, overlap, the logged reads-left numbers, the both-sides flags; the
array form equals the literal loops on 120 random settings (both alphabets, read lengths 4 .. 40, equal reads in a random
order), compares past the last row included; each of the four simplifications of the rule misses the reference, and so does
the serial rule; the conditions the fixtures were made under hold."""
import glob
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

import pgovl_par_util as pp
import pgovl_util as po
from test_pgovl_oracle import assert_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "pgovlpar_*.npz")))
NAMES = ["genome_acgnt_L33", "genome_acgt_L150", "genome_acgt_L40", "lowcomp_acgnt_L40", "lowcomp_acgt_L12", "mixed_acgnt_L40", "no_equal_reads",
         "one_read", "tail_acgnt_L4", "tail_acgnt_L5", "tail_acgt_L4", "tail_acgt_L5", "two_letter_acgnt_L12", "two_letter_acgt_L33"]


def case_name(path):
    return os.path.basename(path)[len("pgovlpar_"):-len(".npz")]


_cache = {}


def load_case(path):
    """the fixture with `codes`, and what the literal loops and the array form give on it; made once and shared: nobody
    writes to it"""
    if path not in _cache:
        z = np.load(path)
        fx = {k: z[k] for k in z.files}
        fx["codes"] = po.to_codes(fx["reads"], int(fx["symbols"]))
        for v in fx.values():
            v.setflags(write=False)
        fx["literal"] = pp.literal(fx["codes"], fx["sorted_order"], float(fx["coef"]), int(fx["symbols"]))
        fx["form"] = pp.parallel_form(fx["codes"], fx["sorted_order"], float(fx["coef"]), int(fx["symbols"]))
        _cache[path] = fx
    return _cache[path]


def make_module():
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)                          # (it imports the serial rule's maker for the ten settings)
    spec = importlib.util.spec_from_file_location("make_golden_pgovl_par", os.path.join(GOLDEN, "make_golden_pgovl_par.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


def test_the_fixtures_are_there():
    assert [case_name(p) for p in FIXTURES] == NAMES


@pytest.mark.parametrize("path", FIXTURES, ids=case_name)
def test_literal_loops_and_array_form_equal_the_reference(path):
    fx = load_case(path)
    L, symbols, coef = int(fx["L"]), int(fx["symbols"]), float(fx["coef"])
    assert np.array_equal(po.pack_rows(fx["reads"], symbols), fx["rows"])
    assert po.order_is_sorted(fx["codes"], fx["sorted_order"])
    lit, form = fx["literal"], fx["form"]
    assert_result(lit, fx, "literal")
    assert lit["reads_left"].size == max(po.iterations(L, coef), 1) and lit["sweeps"] == lit["reads_left"].size - 1
    assert_result(form, lit, "array form")
    assert lit["counters"]["past_end_compares"] == 0 and form["counters"]["past_end_compares"] == 0
    assert np.array_equal(po.both_sides(fx["next_read"], fx["overlap"], L), fx["flags"])
    assert pp.valid_graph(fx["codes"], fx["next_read"], fx["overlap"])


def test_array_form_equals_the_literal_loops_on_120_random_settings():
    total = dict(resets_changing=0, follower_compares=0, past_end_compares=0, glued=0, self_conflicts=0, would_drop=0)
    lengths = set()
    for k in range(120):
        codes, symbols, coef, order = pp.random_case(k)
        lengths.add(codes.shape[1])
        lit = pp.literal(codes, order, coef, symbols)
        form = pp.parallel_form(codes, order, coef, symbols)
        assert_result(form, lit, k)
        assert pp.valid_graph(codes, form["next_read"], form["overlap"]), k
        for c in total:
            total[c] += form["counters"][c]
    assert min(lengths) == 4 and max(lengths) == 40
    assert all(v > 0 for v in total.values()), total


def test_each_simplification_and_the_serial_rule_miss_the_reference():
    mk = make_module()
    manifest = json.load(open(os.path.join(GOLDEN, "manifest_pgovl_par.json")))

    def misses(res, fx):
        return not (np.array_equal(res["next_read"], fx["next_read"]) and np.array_equal(res["overlap"], fx["overlap"].astype(np.uint16))
                    and np.array_equal(res["reads_left"], fx["reads_left"]))

    for name, kw in mk.SIMPLIFICATIONS.items():
        paths = [p for p in FIXTURES if manifest[case_name(p)]["differs_" + name]]
        assert paths, name
        fx = load_case(min(paths, key=os.path.getsize))
        assert misses(pp.parallel_form(fx["codes"], fx["sorted_order"], float(fx["coef"]), int(fx["symbols"]), **kw), fx), name
    differ = [p for p in FIXTURES if manifest[case_name(p)]["differs_serial_rule"]]
    assert len(differ) >= 9
    fx = load_case(min(differ, key=os.path.getsize))
    assert misses(po.literal(fx["codes"], fx["sorted_order"], float(fx["coef"]), int(fx["symbols"])), fx)


def test_manifest_conditions_hold():
    mk = make_module()
    manifest = json.load(open(os.path.join(GOLDEN, "manifest_pgovl_par.json")))
    assert sorted(manifest) == NAMES == sorted(c[0] for c in mk.PAR_CASES)
    for path in FIXTURES:
        name, fx = case_name(path), load_case(path)
        m = manifest[name]
        assert os.path.getsize(path) == m["bytes"] <= mk.MAX_BYTES
        assert (int(fx["L"]), int(fx["symbols"]), float(fx["coef"]), fx["codes"].shape[0]) == (m["L"], m["symbols"], m["coef"], m["reads"])
        assert m["tail_sweeps"] == pp.tail_sweeps(m["L"], m["coef"])
        for k, v in fx["form"]["counters"].items():
            assert m[k] == v, (name, k)
        assert m["reference_follower_compares"] == fx["literal"]["counters"]["follower_compares"]
    mk.check_set(manifest)


def test_the_follower_key_orders_by_the_rows_behind_a_read():
    codes = np.array([[0, 1, 2, 3], [0, 0, 0, 0], [3, 3, 3, 3], [0, 0, 0, 0], [3, 3, 3, 3]], dtype=np.uint8)
    fk = pp.FollowerKey(pp.dense_read_ranks(codes, po.stable_order(codes)))
    assert fk.cmp(1, 2) < 0 and fk.cmp(2, 1) > 0            # AAAA behind read 1, TTTT behind read 2
    assert (fk.compares, fk.past_end) == (2, 0)
    assert fk.cmp(2, 4) > 0                                 # equal followers (TTTT), then AAAA against no row: the rows of 4 end first
    assert fk.cmp(5, 1) < 0 and (fk.compares, fk.past_end) == (4, 2)
