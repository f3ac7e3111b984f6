"""The checker of the pseudogenome assembly against the reference, without a GPU: tests/pgasm_util's literal loops give what
the compiled reference gave for every fixture of tests/golden/make_golden_pgasm.py, byte for byte and number for number;
the parallel form the device runs equals the literal loops on 300 random settings (duplicates, cycles on circular texts
shorter than a read, read lengths from 1 to 23, both alphabets); and the conditions the fixtures were made under hold."""
import glob
import json
import os

import numpy as np
import pytest

import pgasm_util as pa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "pgasm_*.npz")))
NUMBERS = ("pg_len", "cycles", "overlap_lost", "components", "singles")


def case_name(path):
    return os.path.basename(path)[len("pgasm_"):-len(".npz")]


def load_case(path):
    z = np.load(path)
    fx = {k: z[k] for k in z.files}
    fx["reads"] = pa.unpack_rows(fx["rows"], int(fx["L"]), int(fx["symbols"]))
    return fx


def assert_result(got, want, what=""):
    for k in NUMBERS:
        assert int(got[k]) == int(want[k]), (what, k, int(got[k]), int(want[k]))
    for k, dt in (("text", np.uint8), ("off", np.uint16), ("org_idx", np.uint32)):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == np.dtype(dt) and g.size == w.size, (what, k, g.dtype, g.size, w.size)
        assert g.tobytes() == w.astype(dt).tobytes(), (what, k)


def test_the_fixtures_are_there():
    assert [case_name(p) for p in FIXTURES] == ["mixed_acgnt", "mixed_acgt", "no_overlap", "one_read"]


@pytest.mark.parametrize("path", FIXTURES, ids=case_name)
def test_literal_loops_equal_the_reference(path):
    fx = load_case(path)
    assert np.array_equal(pa.pack_rows(fx["reads"], int(fx["symbols"])), fx["rows"])
    nx, ov, head, cycles, lost, _ = pa.literal_remove_cycles(fx["next_read"], fx["overlap"])
    assert np.array_equal(nx[1:], fx["next_read_cut"][1:]) and np.array_equal(ov[1:], fx["overlap_cut"][1:])
    assert np.array_equal(head[1:], fx["head_read"][1:])
    assert (cycles, lost) == (int(fx["cycles"]), int(fx["overlap_lost"]))
    assert_result(pa.literal(fx["reads"], fx["next_read"], fx["overlap"]), fx, "literal")
    assert_result(pa.parallel_form(fx["reads"], fx["next_read"], fx["overlap"]), fx, "parallel")
    assert pa.links_are_real(fx["reads"], fx["next_read"], fx["overlap"])


def random_setting(k):
    rng = np.random.default_rng(1000 + k)
    L = int(rng.integers(1, 24))
    symbols = 4 if k % 2 else 5
    nch, ncy = int(rng.integers(0, 6)), int(rng.integers(0, 5))
    return dict(seed=k, L=L, symbols=symbols, chains=rng.integers(1, 40, size=nch).tolist(), cycles=rng.integers(1, 12, size=ncy).tolist(),
                singles=int(rng.integers(0 if nch + ncy else 1, 6)), dup=float(rng.choice([0.0, 0.1, 0.5])), mean_shift=int(rng.integers(1, L + 1)),
                n_share=0.05, ov_dtype=np.uint8 if k % 3 else np.uint16)


def test_parallel_form_equals_the_literal_loops_on_300_random_settings():
    seen_cycles = seen_short = seen_dups = 0
    for k in range(300):
        s = random_setting(k)
        c = pa.make_case(**s)
        assert pa.links_are_real(c["reads"], c["next_read"], c["overlap"]), s
        R = c["reads"].shape[0]
        mapping = np.random.default_rng(k).permutation(R).astype(np.uint32) if k % 2 else None
        lit = pa.literal(c["reads"], c["next_read"], c["overlap"], mapping)
        par = pa.parallel_form(c["reads"], c["next_read"], c["overlap"], mapping)
        assert_result(par, lit, s)
        assert sorted(lit["cuts"]) == par["cuts"], s
        assert lit["cycles"] == len(s["cycles"]), s
        assert np.array_equal(pa.unpack_rows(c["rows"], s["L"], s["symbols"]), c["reads"])
        seen_cycles += lit["cycles"]
        seen_dups += int((c["overlap"][1:] == s["L"]).sum())
        seen_short += int(lit["overlap_lost"] > 0 and s["L"] > 4)
    assert seen_cycles > 300 and seen_dups > 1000 and seen_short > 50


def test_every_cut_is_at_the_largest_index_of_its_cycle():
    for k in range(40):
        c = pa.make_case(seed=k, L=12, chains=[5, 9], cycles=[1, 2, 3, 17, 40], singles=3, dup=0.1)
        nx0 = c["next_read"]
        lit = pa.literal(c["reads"], nx0, c["overlap"])
        for m in lit["cuts"]:
            members, j = [m], int(nx0[m])
            while j != m:
                members.append(j)
                j = int(nx0[j])
            assert m == max(members)


def test_manifest_conditions_hold():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_pgasm", os.path.join(GOLDEN, "make_golden_pgasm.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    manifest = json.load(open(os.path.join(GOLDEN, "manifest_pgasm.json")))
    assert sorted(manifest) == sorted(case_name(p) for p in FIXTURES) == sorted(c[0] for c in mk.PGASM_CASES)
    for path in FIXTURES:
        name, fx = case_name(path), load_case(path)
        m = manifest[name]
        c = mk.conditions(fx)
        assert {k: m[k] for k in c} == c, name
        assert c["cuts"] == c["cycles"] == c["cuts_at_largest"]
        assert os.path.getsize(path) == m["bytes"] <= mk.MAX_BYTES
        if m["mixed"]:
            mk.check_mixed(name, c)
    assert manifest["mixed_acgnt"]["reads_with_n"] >= 3 and manifest["mixed_acgnt"]["L"] % 3
    assert manifest["no_overlap"]["singles"] == manifest["no_overlap"]["reads"]
    assert manifest["one_read"]["reads"] == 1
