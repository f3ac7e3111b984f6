"""The pair-position coding of the order-preserving paired mode, pinned on the CPU: tests/pairpos_util's literal restatement
of compressReadsPgPositions / decompressReadsPgPositions reproduces the reference-made fixtures byte for byte in both
directions, round-trips random generator settings, and agrees with the three-state form of the chain that the device
runs (pgrc_amd/csrc/pairpos.hip); the library exports the new entry points (no compute call: no GPU needed)."""
import glob
import json
import os
import re

import numpy as np
import pytest

import pairpos_util as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "pairpos_*.npz")))


def load_case(path):
    """-> (input positions interleaved, the reference's streams as a dict, its decoded array as uint64, the knobs)"""
    z = np.load(path)
    W, pairs = int(z["pos_width"]), int(z["pairs"])
    st = {"n_total": 2 * pairs, "pos_width": W}
    for k in pp.STREAMS:
        st[k] = z[k]
    return z["org"], st, z["decoded"].astype(np.uint64), json.loads(z["knobs"].tobytes().decode())


def random_setting(seed):
    """(pairs, W, generator knobs) of random setting number `seed`"""
    rng = np.random.default_rng(10_000 + seed)
    pairs = int(rng.choice([int(rng.integers(0, 4)), int(rng.integers(4, 200)), int(rng.integers(200, 4000))], p=[0.2, 0.3, 0.5]))
    knobs = dict(near=float(rng.choice([0.0, 1.0, *(0.8 * rng.random(4))])), jump=float(rng.random() * 0.6), ret=float(rng.random() * 0.3),
                 tie=float(rng.choice([0.0, rng.random() * 0.5])), special=float(rng.random() * 0.3),
                 drift=int(rng.choice([0, 100, 2000, 20000, 40000])), hi=bool(rng.integers(0, 2)))
    return pairs, (4, 8)[seed % 2], knobs


def test_fixtures_are_present_and_hold_every_kind():
    names = {os.path.basename(f) for f in FIXTURES}
    assert {"pairpos_w4_mixed.npz", "pairpos_w8_above_4g.npz", "pairpos_all_near.npz", "pairpos_all_far.npz",
            "pairpos_ties_boundaries.npz"} <= names
    manifest = json.load(open(os.path.join(GOLDEN, "manifest_pairpos.json")))
    largest = max(os.path.getsize(f) for f in glob.glob(os.path.join(GOLDEN, "pgmap_*.npz")))
    for path in FIXTURES:
        name = os.path.basename(path)[8:-4]
        org, st, _, knobs = load_case(path)
        m = manifest[name]
        assert os.path.getsize(path) <= largest
        counts = dict(pp.kinds(st), ties=pp.ties(org))
        assert {k: m[k] for k in counts} == counts
        if m["mixed"]:
            assert min(counts.values()) >= 50, (name, counts)
        # the stored positions are the generator's
        assert np.array_equal(org, pp.make_positions(int(np.load(path)["seed"]), m["pairs"], m["pos_width"], **knobs))
    assert manifest["w8_above_4g"]["above_4g"] > 1000


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def test_literal_encoder_reproduces_the_reference_streams(path):
    org, st, _, _ = load_case(path)
    got = pp.compress_literal(org, st["pos_width"])
    for k in pp.STREAMS:
        assert got[k].dtype == st[k].dtype and got[k].tobytes() == st[k].tobytes(), k


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def test_literal_decoder_reproduces_the_reference_array(path):
    org, st, decoded, _ = load_case(path)
    got = pp.decompress_literal(st)
    assert got.tobytes() == decoded.tobytes()
    assert np.array_equal(got, pp.file_major(org))


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def test_three_state_form_reproduces_the_reference_streams(path):
    org, st, _, _ = load_case(path)
    assert pp.streams_equal(pp.compress_states(org, st["pos_width"]), st)


@pytest.mark.parametrize("block", range(10))
def test_round_trip_and_three_state_form_on_random_settings(block):
    """30 settings per block: decode(encode(x)) is x in file-major layout, and the scan of state maps gives the literal
    loop's streams -- the CPU proof that the device's formulation is the reference's rule"""
    seen = {"near": 0, "delta": 0, "full_set": 0, "full_keep": 0}
    for seed in range(30 * block, 30 * block + 30):
        pairs, W, knobs = random_setting(seed)
        org = pp.make_positions(seed, pairs, W, **knobs)
        lit = pp.compress_literal(org, W)
        assert np.array_equal(pp.decompress_literal(lit), pp.file_major(org)), (seed, pairs, W, knobs)
        assert pp.streams_equal(pp.compress_states(org, W), lit), (seed, pairs, W, knobs)
        for k, v in pp.kinds(lit).items():
            seen[k] += v
    assert min(seen.values()) > 100, seen


def test_boundary_values_by_hand():
    """rel 65535 / 65536, deltas 32767 / 32768 / -32768 / -32769, mate == base, equal bases: the kinds by hand"""
    b = 1 << 20
    near = [(b, b), (b + 1, b + 1 + 65535)]             # mate == base: near, not base-first; rel 65535: near
    # far pairs in rank order, by rel: SET (the first far pair; 65536 is far), delta +32767 twice, +32768 is a full pair that
    # KEEPS refPrev = 131070, -32768 against the kept value is a delta pair (against the pair before it would be -65536),
    # a full pair after it KEEPS again, the next one is judged against the kept 98302 and SETS, -32769 is a full pair
    # that SETS, and -32768 with the mate before the base is a delta pair
    rels = [65536, 98303, 131070, 163838, 98302, 198302, 198307, 165538, 132770]
    far = [(b + 2 + k, b + 2 + k + r) for k, r in enumerate(rels[:-1])] + [(b + 20, b + 20 - rels[-1])]
    far[5] = (far[4][0], far[4][0] + rels[5])           # equal bases: the pair number decides
    org = np.array([v for p in near + far for v in p], dtype=np.uint64)
    st = pp.compress_literal(org, 4)
    assert st["off16_flag"].tolist() == [1, 1] + [0] * 9
    assert st["off_base_first"].tolist() == [0, 1] and st["off_value"].tolist() == [0, 65535]
    assert st["delta16_flag"].tolist() == [0, 1, 1, 0, 1, 0, 0, 0, 1]
    assert st["delta_value"].tolist() == [32767, 32767, -32768, -32768] and st["delta_base_first"].tolist() == [1, 1, 1, 0]
    assert st["not_base_pos"].tolist() == [far[k][1] for k in (0, 3, 5, 6, 7)]
    assert pp.kinds(st) == {"near": 2, "delta": 4, "full_set": 3, "full_keep": 2}
    assert pp.streams_equal(pp.compress_states(org, 4), st)
    assert np.array_equal(pp.decompress_literal(st), pp.file_major(org))


def test_library_exports_the_pair_position_entry_points():
    from pgrc_amd import _lib, decode
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgrc_decode.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pgrc_(?:pairpos|decode)_\w+)\s*\(", txt))
    want = {"pgrc_pairpos_encode", "pgrc_pairpos_free", "pgrc_pairpos_decode", "pgrc_decode_set_order_pair_streams",
            "pgrc_pairpos_get_timing"}
    assert want <= declared
    for s in want:
        assert hasattr(_lib.lib, s), f"{s} is not exported by libpgrc_match.so"
    assert want <= {name for name, _, _ in decode.DECODE_PROTOS}
    import pgrc_amd
    assert callable(pgrc_amd.compressReadsPgPositions) and callable(pgrc_amd.decompressReadsPgPositions)
    assert callable(pgrc_amd.PgRCDecoder.set_order_pair_streams)
