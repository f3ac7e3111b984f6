"""The pair-order coding of the paired mode that does not preserve the order, pinned on the CPU: tests/pairorder_util's literal
restatement of compressReadsOrder / decompressReadsOrder reproduces the reference-made fixtures byte for byte in every form,
the parallel form that the device runs (pgrc_amd/csrc/pairorder.hip) agrees with the literal loop on 300 random settings,
and the decoded orders bring every pair together; the library exports the new entry points (no compute call: no GPU
needed)."""
import glob
import json
import os
import re

import numpy as np
import pytest

import pairorder_util as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "pairorder_*.npz")))
KINDS = ("near", "delta", "full_set", "full_keep")
BOUNDS = ("rel_255", "rel_256", "delta_127", "delta_m128")


def case_name(path):
    return os.path.basename(path)[len("pairorder_"):-4]


def load_case(path):
    """-> (org, the reference's streams as a dict, its decoded rlIdxOrder, seed, the knobs)"""
    z = np.load(path)
    form, pairs = int(z["form"]), int(z["pairs"])
    st = {"n_total": 2 * pairs, "form": form}
    for k, _ in po.stream_types(form):
        st[k] = z[k]
    return z["org"], st, z["decoded"], int(z["seed"]), json.loads(z["knobs"].tobytes().decode())


def random_setting(seed):
    """(pairs, form, generator knobs) of random setting number `seed`"""
    rng = np.random.default_rng(20_000 + seed)
    pairs = int(rng.choice([int(rng.integers(0, 4)), int(rng.integers(4, 200)), int(rng.integers(200, 3000))], p=[0.2, 0.3, 0.5]))
    knobs = dict(near=float(rng.choice([0.0, 1.0, *(0.8 * rng.random(4))])), jump=float(rng.random() * 0.6), ret=float(rng.random() * 0.3),
                 special=float(rng.random() * 0.3), drift=int(rng.choice([0, 10, 100, 127, 128, 300])),
                 span=int(rng.choice([300, 1 << 10, 1 << 14])), exact=bool(rng.random() < 0.7))
    return pairs, po.FORMS[seed % 4], knobs


def test_fixtures_are_present_and_hold_every_kind():
    names = {case_name(f) for f in FIXTURES}
    assert {"mixed_ignore", "mixed_file_flags", "mixed_complete", "mixed_complete_single_file", "all_near", "all_far",
            "boundaries", "one_pair"} <= names
    manifest = json.load(open(os.path.join(GOLDEN, "manifest_pairorder.json")))
    largest = max(os.path.getsize(f) for f in glob.glob(os.path.join(GOLDEN, "pgmap_*.npz")))
    forms = set()
    for path in FIXTURES:
        name = case_name(path)
        org, st, _, seed, knobs = load_case(path)
        m = manifest[name]
        assert os.path.getsize(path) <= largest
        assert m["form"] == st["form"] and 2 * m["pairs"] == st["n_total"] == org.size
        # (the single-file form writes rev alone: its kinds are those of the same order in the COMPLETE form)
        coded = st if st["form"] != po.COMPLETE_SINGLE_FILE else po.compress_literal(org, po.COMPLETE)
        counts = dict(po.kinds(coded), **po.boundaries(coded))
        assert {k: m[k] for k in counts} == counts
        if m["mixed"]:
            forms.add(st["form"])
            assert min(counts[k] for k in KINDS) >= 50, (name, counts)
            assert min(counts[k] for k in BOUNDS) >= 1, (name, counts)
            if st["form"] == po.FILE_FLAGS:
                for k in ("off_base_file_flag", "nonoff_base_file_flag"):
                    assert set(np.unique(st[k]).tolist()) == {0, 1}, (name, k)
        assert np.array_equal(org, po.make_order(seed, m["pairs"], **knobs))     # the stored order is the generator's
    assert forms == set(po.FORMS)
    assert manifest["all_near"]["near"] == manifest["all_near"]["pairs"] and manifest["all_far"]["near"] == 0
    assert manifest["one_pair"]["pairs"] == 1


@pytest.mark.parametrize("path", FIXTURES, ids=case_name)
def test_literal_encoder_reproduces_the_reference_streams(path):
    org, st, _, _, _ = load_case(path)
    got = po.compress_literal(org, st["form"])
    assert set(got) == set(st)
    for k, _ in po.stream_types(st["form"]):
        assert got[k].dtype == st[k].dtype and got[k].tobytes() == st[k].tobytes(), k


@pytest.mark.parametrize("path", FIXTURES, ids=case_name)
def test_parallel_form_reproduces_the_reference_streams(path):
    org, st, _, _, _ = load_case(path)
    assert po.streams_equal(po.compress_parallel(org, st["form"]), st)


@pytest.mark.parametrize("path", FIXTURES, ids=case_name)
def test_literal_decoder_reproduces_the_reference_order_and_the_pairs(path):
    org, st, decoded, _, _ = load_case(path)
    got = po.decompress_literal(po.compress_literal(org, st["form"]))
    assert got.dtype == decoded.dtype and got.tobytes() == decoded.tobytes()
    rev = np.empty(org.size, np.uint32)
    rev[org] = np.arange(org.size, dtype=np.uint32)
    if st["form"] in (po.COMPLETE, po.COMPLETE_SINGLE_FILE):
        assert np.array_equal(got, rev)
    else:
        assert po.pairs_are_mates(got, org)
    if st["form"] == po.FILE_FLAGS:             # file 1 gets the even read of every pair, file 2 the odd one
        o = org[got]
        assert (o[0::2] % 2 == 0).all() and np.array_equal(o[1::2], o[0::2] + 1)
    if st["form"] == po.IGNORE:                 # the base first, the bases in entry order
        assert (got[0::2] < got[1::2]).all() and (np.diff(got[0::2].astype(np.int64)) > 0).all()


@pytest.mark.parametrize("block", range(10))
def test_parallel_form_equals_the_literal_loop_on_random_settings(block):
    """30 settings per block: the device's formulation gives the literal loop's streams, and the literal decoder brings
    every pair back together -- the CPU proof that the formulation is the reference's rule"""
    seen = dict.fromkeys(KINDS, 0)
    for seed in range(30 * block, 30 * block + 30):
        pairs, form, knobs = random_setting(seed)
        org = po.make_order(seed, pairs, **knobs)
        assert np.array_equal(np.sort(org), np.arange(2 * pairs)), (seed, pairs, knobs)
        lit = po.compress_literal(org, form)
        assert po.streams_equal(po.compress_parallel(org, form), lit), (seed, pairs, form, knobs)
        order = po.decompress_literal(lit)
        if form in (po.COMPLETE, po.COMPLETE_SINGLE_FILE):
            assert np.array_equal(org[order], np.arange(2 * pairs)), (seed, pairs, form, knobs)
        else:
            assert po.pairs_are_mates(order, org), (seed, pairs, form, knobs)
        if form == po.FILE_FLAGS:
            assert (org[order][0::2] % 2 == 0).all(), (seed, pairs, knobs)
        if form != po.COMPLETE_SINGLE_FILE:
            for k, v in po.kinds(lit).items():
                seen[k] += v
    assert min(seen.values()) > 100, seen


def test_boundary_values_by_hand():
    """rel 255 / 256 and deltas 127 / 128 / -128 / -129: the kinds by hand.  Bases at entries 0 .. 8 (in entry order), their
    mates further on, every other entry paired with its neighbour behind them."""
    rels = [255, 256, 383, 511, 300, 1000, 1005, 876, 748]
    # 256: the first far pair SETS (256 - 0 does not fit); +127 delta; +128 is a full pair that KEEPS refPrev = 383; 300 is -83
    # against the kept value, a delta pair (against the pair before it would be -211); 1000 full after a delta KEEPS 300;
    # 1005 is judged against the kept 300 and SETS; -129 is a full pair that SETS; -128 is a delta pair
    T = 4000
    org = np.full(T, -1, np.int64)
    for k, r in enumerate(rels):
        org[k], org[k + r] = 2 * k, 2 * k + 1
    rest = np.flatnonzero(org < 0)
    org[rest] = 2 * len(rels) + np.arange(rest.size)
    st = po.compress_literal(org.astype(np.uint32), po.FILE_FLAGS)
    assert st["off8_flag"][:9].tolist() == [1] + [0] * 8 and st["off_value"][0] == 255
    assert st["delta8_flag"].tolist() == [0, 1, 0, 1, 0, 0, 0, 1] and st["delta_value"].tolist() == [127, -83, -128]
    assert st["full_offset"].tolist() == [256, 511, 1000, 1005, 876]
    assert po.kinds(st)["full_keep"] == 2 and po.kinds(st)["full_set"] == 3
    assert st["off_base_file_flag"][:1].tolist() == [0] and not st["nonoff_base_file_flag"].any()
    assert po.streams_equal(po.compress_parallel(org.astype(np.uint32), po.FILE_FLAGS), st)


def test_library_exports_the_pair_order_entry_points():
    from pgrc_amd import _lib, decode
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgrc_decode.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pgrc_pairorder_\w+)\s*\(", txt))
    want = {"pgrc_pairorder_encode", "pgrc_pairorder_free", "pgrc_pairorder_get_timing"}
    assert want == declared
    for s in want:
        assert hasattr(_lib.lib, s), f"{s} is not exported by libpgrc_match.so"
    assert want <= {name for name, _, _ in decode.DECODE_PROTOS}
    import pgrc_amd
    assert callable(pgrc_amd.compressReadsOrder) and callable(pgrc_amd.PgRCDecoder.compressReadsOrder)
    assert callable(pgrc_amd.PgRCDecoder.pairorder_timing)
    assert [decode.PGRC_PAIRORDER_IGNORE, decode.PGRC_PAIRORDER_FILE_FLAGS, decode.PGRC_PAIRORDER_COMPLETE,
            decode.PGRC_PAIRORDER_COMPLETE_SINGLE_FILE] == list(po.FORMS)
