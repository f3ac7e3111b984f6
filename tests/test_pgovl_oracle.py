"""The checker of the overlap search against the reference, without a GPU: tests/pgovl_util's literal loops give what the
compiled reference gave for every fixture of tests/golden/make_golden_pgovl.py -- nextRead, overlap, the logged reads-left
numbers, the both-sides flags; the parallel form the device runs equals the literal loops on the fixtures and on 120 random
settings (genome-like, periodic and mixed reads, both alphabets, read lengths 4 .. 40, three stop coefficients, equal reads in
a random order); each of the three simplifications of the rule misses the reference; the associative form of the groups' order
equals the step-by-step form and the closed form of the pairing equals its automaton; the conditions the fixtures were made
under hold; and, where the compiled reference and its tree are present, the parallel form equals it on fresh random cases."""
import glob
import importlib.util
import json
import os
import tempfile

import numpy as np
import pytest

import pgovl_util as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "pgovl_*.npz")))
NAMES = ["genome_acgnt_L33", "genome_acgt_L150", "genome_acgt_L40", "lowcomp_acgnt_L40", "lowcomp_acgt_L12", "mixed_acgnt_L40", "no_equal_reads",
         "one_read", "two_letter_acgnt_L12", "two_letter_acgt_L33"]


def case_name(path):
    return os.path.basename(path)[len("pgovl_"):-len(".npz")]


_cache = {}


def load_case(path):
    """the fixture with `codes` (the symbols' places); loaded once and shared: nobody writes to it"""
    if path not in _cache:
        z = np.load(path)
        fx = {k: z[k] for k in z.files}
        fx["codes"] = po.to_codes(fx["reads"], int(fx["symbols"]))
        for v in fx.values():
            v.setflags(write=False)
        _cache[path] = fx
    return _cache[path]


def assert_result(got, want, what=""):
    """next_read, overlap, the reads-left numbers (and, where `want` has them, the three counts)"""
    assert np.array_equal(got["next_read"], want["next_read"]), (what, "next_read")
    assert np.array_equal(np.asarray(got["overlap"], dtype=np.uint16), np.asarray(want["overlap"], dtype=np.uint16)), (what, "overlap")
    assert np.array_equal(np.asarray(got["reads_left"], dtype=np.uint64), np.asarray(want["reads_left"], dtype=np.uint64)), (what, "reads_left")
    for k in ("duplicates", "links", "sweeps"):
        if k in want:
            assert int(got[k]) == int(want[k]), (what, k, int(got[k]), int(want[k]))


def make_module():
    spec = importlib.util.spec_from_file_location("make_golden_pgovl", os.path.join(GOLDEN, "make_golden_pgovl.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


def test_the_fixtures_are_there():
    assert [case_name(p) for p in FIXTURES] == NAMES


@pytest.mark.parametrize("path", FIXTURES, ids=case_name)
def test_literal_loops_and_parallel_form_equal_the_reference(path):
    fx = load_case(path)
    L, symbols, coef = int(fx["L"]), int(fx["symbols"]), float(fx["coef"])
    assert np.array_equal(po.pack_rows(fx["reads"], symbols), fx["rows"])
    assert po.order_is_sorted(fx["codes"], fx["sorted_order"])
    lit = po.literal(fx["codes"], fx["sorted_order"], coef, symbols)
    assert_result(lit, fx, "literal")
    assert lit["reads_left"].size == max(po.iterations(L, coef), 1) and lit["sweeps"] == lit["reads_left"].size - 1
    par = po.parallel_form(fx["codes"], fx["sorted_order"], coef)
    assert_result(par, lit, "parallel")
    assert np.array_equal(po.both_sides(fx["next_read"], fx["overlap"], L), fx["flags"])


def test_parallel_form_equals_the_literal_loops_on_120_random_settings():
    total = dict(tie_runs_off_symbol_order=0, round_robin_runs=0, self_conflicts=0, dropped=0)
    for k in range(120):
        codes, symbols, coef, order = po.random_case(k)
        assert po.order_is_sorted(codes, order)
        lit = po.literal(codes, order, coef, symbols)
        par = po.parallel_form(codes, order, coef)
        assert_result(par, lit, k)
        for c in total:
            total[c] += par["counters"][c]
    assert total["tie_runs_off_symbol_order"] > 100 and total["round_robin_runs"] > 30 and total["self_conflicts"] > 100 and total["dropped"] > 100, total


def test_each_simplification_misses_the_reference():
    mk = make_module()
    manifest = json.load(open(os.path.join(GOLDEN, "manifest_pgovl.json")))
    for name, kw in mk.SIMPLIFICATIONS.items():
        missed = 0
        for path in FIXTURES:
            if not manifest[case_name(path)]["differs_" + name]:
                continue
            fx = load_case(path)
            alt = po.parallel_form(fx["codes"], fx["sorted_order"], float(fx["coef"]), **kw)
            assert not (np.array_equal(alt["next_read"], fx["next_read"]) and np.array_equal(alt["overlap"], fx["overlap"].astype(np.uint16))), (name, case_name(path))
            missed += 1
            if missed == 2:
                break
        assert missed, name


def test_associative_order_and_closed_form_pairing():
    rng = np.random.default_rng(11)
    for _ in range(1500):
        n = int(rng.integers(1, 14))
        keys = rng.integers(0, 4, size=(n, po.GROUPS)) * (rng.random((n, po.GROUPS)) < 0.6)
        assert np.array_equal(po.states_before(po.SYMBOL_ORDER, keys), po.compose_steps(po.SYMBOL_ORDER, keys))
        a, b, c = (po.dense(rng.integers(0, 3, size=(1, po.GROUPS))) for _ in range(3))
        assert np.array_equal(po.compose(po.compose(a, b), c), po.compose(a, po.compose(b, c)))
        zero = np.zeros((1, po.GROUPS), dtype=np.int64)
        assert np.array_equal(po.compose(a, zero), a) and np.array_equal(po.compose(zero, a), a)
        e = rng.random(24) < 0.6
        start = rng.random(24) < 0.2
        start[0] = True
        assert np.array_equal(po.events_closed_form(e, start), po.events_automaton(e, start))


def test_manifest_conditions_hold():
    mk = make_module()
    manifest = json.load(open(os.path.join(GOLDEN, "manifest_pgovl.json")))
    assert sorted(manifest) == NAMES == sorted(c[0] for c in mk.PGOVL_CASES)
    for path in FIXTURES:
        name, fx = case_name(path), load_case(path)
        m = manifest[name]
        assert os.path.getsize(path) == m["bytes"] <= mk.MAX_BYTES
        assert (int(fx["L"]), int(fx["symbols"]), float(fx["coef"]), fx["codes"].shape[0]) == (m["L"], m["symbols"], m["coef"], m["reads"])
        if name in ("genome_acgt_L40", "lowcomp_acgt_L12", "no_equal_reads"):       # (the counters of every fixture: the generator's own run)
            c = mk.conditions(fx)
            assert {k: m[k] for k in c} == c, name
    mk.check_set(manifest)


def test_parallel_form_equals_the_compiled_reference_on_fresh_cases():
    mk = make_module()
    if not (os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libpgrc_ref.so")) and os.path.isdir(os.path.join(mk.REF, "pseudogenome"))):
        return                                              # (the fixtures are what the reference gave where it was present)
    with tempfile.TemporaryDirectory() as tmp:
        exe = mk.build_driver(tmp)
        for k in range(12):
            codes, symbols, coef, _ = po.random_case(900 + k)
            L = codes.shape[1]
            fx = mk.reference_run(exe, tmp, po.ascii_of(codes, symbols), L, symbols, coef)
            par = po.parallel_form(codes, fx["sorted_order"], coef)
            assert_result(par, fx, k)
            assert np.array_equal(po.both_sides(par["next_read"], par["overlap"], L), fx["flags"])
