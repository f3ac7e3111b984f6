"""tests/verify_util.py, the CPU side of the verifier's tests: both rules on hand-written cases whose answers are written out
here, the numpy key against a per-item loop over Python integers, the pairing under given keys, and the seed of the 20-bit
collision case that tests/test_gpu_verify.py runs on the device."""
import numpy as np
import pytest

import verify_util as vu

N64, N32 = vu.NONE64, vu.NONE32


def rows(*words):
    return np.array([list(w.encode()) for w in words], np.uint8).reshape(len(words), -1)


def want(kind, ok, ns, nd, **kw):
    r = {"kind": kind, "ok": ok, "salts_used": 1 if kind == vu.MULTISET else 0, "n_source": ns, "n_decoded": nd, "mismatched_rows": 0,
         "first_mismatch_file": N32, "first_mismatch_row": N64, "source_unmatched": 0, "decoded_unmatched": 0, "undecided": 0,
         "first_source_unmatched": N64, "first_decoded_unmatched": N64}
    r.update(kw)
    return r


DEC = rows("ACGT", "CCCC", "GATT", "ACGT", "TTTT")


def test_equal_sides():
    assert vu.verify_in_order([DEC], [DEC]) == want(vu.IN_ORDER, True, [5, 0], [5, 0])
    assert vu.verify_multiset([DEC[::-1]], [DEC]) == want(vu.MULTISET, True, [5, 0], [5, 0])
    e = np.zeros((0, 4), np.uint8)
    assert vu.verify_multiset([e], [e]) == want(vu.MULTISET, True, [0, 0], [0, 0], salts_used=0)
    assert vu.verify_in_order([e], [e]) == want(vu.IN_ORDER, True, [0, 0], [0, 0])


def test_a_flip():
    src = DEC.copy()
    src[2, 3] = ord("A")                # GATT -> GATA
    assert vu.verify_in_order([src], [DEC]) == want(vu.IN_ORDER, False, [5, 0], [5, 0], mismatched_rows=1, first_mismatch_file=0, first_mismatch_row=2)
    assert vu.verify_multiset([src], [DEC]) == want(vu.MULTISET, False, [5, 0], [5, 0], source_unmatched=1, decoded_unmatched=1,
                                                    first_source_unmatched=2, first_decoded_unmatched=2)


def test_a_swap():
    src = DEC[[0, 2, 1, 3, 4]]
    assert vu.verify_in_order([src], [DEC]) == want(vu.IN_ORDER, False, [5, 0], [5, 0], mismatched_rows=2, first_mismatch_file=0, first_mismatch_row=1)
    assert vu.verify_multiset([src], [DEC]) == want(vu.MULTISET, True, [5, 0], [5, 0])


def test_a_drop():
    src = DEC[[0, 1, 3, 4]]             # GATT is gone
    assert vu.verify_in_order([src], [DEC]) == want(vu.IN_ORDER, False, [4, 0], [5, 0], mismatched_rows=2, first_mismatch_file=0, first_mismatch_row=2)
    assert vu.verify_multiset([src], [DEC]) == want(vu.MULTISET, False, [4, 0], [5, 0], decoded_unmatched=1, first_decoded_unmatched=2)


def test_multiplicity_two_against_one():
    src = DEC[[0, 1, 2, 4]]             # one ACGT where the job has two: the job's LAST one (row 3) has no partner
    assert vu.verify_multiset([src], [DEC]) == want(vu.MULTISET, False, [4, 0], [5, 0], decoded_unmatched=1, first_decoded_unmatched=3)
    src = DEC[[0, 1, 2, 3, 4, 0, 0]]    # four against two: the last two of the source
    assert vu.verify_multiset([src], [DEC]) == want(vu.MULTISET, False, [7, 0], [5, 0], source_unmatched=2, first_source_unmatched=5)


def test_two_files_and_unequal_files():
    d0, d1 = DEC[:4], rows("AAAA", "CCCC", "GGGG", "TTTT")
    assert vu.verify_in_order([d0, d1], [d0, d1]) == want(vu.IN_ORDER, True, [4, 4], [4, 4])
    # the mates of pair 1 exchanged between the files: another item
    s0, s1 = d0.copy(), d1.copy()
    s0[1], s1[1] = d1[1], d0[1]
    assert vu.verify_multiset([s0, s1], [d0, d1]) == want(vu.MULTISET, True, [4, 4], [4, 4])     # (both mates are CCCC)
    s0, s1 = d0.copy(), d1.copy()
    s0[2], s1[2] = d1[2], d0[2]
    assert vu.verify_multiset([s0, s1], [d0, d1]) == want(vu.MULTISET, False, [4, 4], [4, 4], source_unmatched=1, decoded_unmatched=1,
                                                          first_source_unmatched=2, first_decoded_unmatched=2)
    assert vu.verify_in_order([s0, s1], [d0, d1]) == want(vu.IN_ORDER, False, [4, 4], [4, 4], mismatched_rows=2, first_mismatch_file=0, first_mismatch_row=2)
    # a whole pair moved: the same multiset, other rows
    p = [1, 2, 3, 0]
    assert vu.verify_multiset([d0[p], d1[p]], [d0, d1])["ok"]
    assert vu.verify_in_order([d0[p], d1[p]], [d0, d1])["mismatched_rows"] == 7 and vu.verify_in_order([d0[p], d1[p]], [d0, d1])["first_mismatch_file"] == 0
    # file 1 one row short: three source items; the job's item 3 has no partner; the counts differ
    assert vu.verify_multiset([d0, d1[:3]], [d0, d1]) == want(vu.MULTISET, False, [4, 3], [4, 4], decoded_unmatched=1, first_decoded_unmatched=3)
    assert vu.verify_in_order([d0, d1[:3]], [d0, d1]) == want(vu.IN_ORDER, False, [4, 3], [4, 4])
    # a mismatch in file 1 of an earlier row comes before one in file 0 of a later row; in one row file 0 comes first
    s0, s1 = d0.copy(), d1.copy()
    s0[3, 0], s1[1, 0] = ord("N"), ord("N")
    assert vu.verify_in_order([s0, s1], [d0, d1]) == want(vu.IN_ORDER, False, [4, 4], [4, 4], mismatched_rows=2, first_mismatch_file=1, first_mismatch_row=1)
    # rows of the job with their newline
    assert vu.verify_in_order([d0], [np.concatenate([d0, np.full((4, 1), 10, np.uint8)], axis=1)], L=4)["ok"]


@pytest.mark.parametrize("L", [1, 7, 8, 9, 150, 255, 300, 510])      # 300 = 2 x 150 and 510 = 2 x 255: items of two files
def test_numpy_key_equals_the_loop(L):
    rng = np.random.default_rng(L)
    items = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, size=(40, L))]
    for salt in (0, 1, 2):
        k = vu.hash_items(items, salt)
        assert k.dtype == np.uint64 and [int(x) for x in k] == [vu.hash_item_loop(it, salt) for it in items]
    assert np.array_equal(vu.hash_items(items, 1, 20), vu.hash_items(items, 1) & np.uint64(0xFFFFF))
    # the words' places count: two words exchanged give another key
    if L >= 16:
        sw = items.copy()
        sw[:, :8], sw[:, 8:16] = items[:, 8:16], items[:, :8]
        differ = (sw != items).any(axis=1)
        assert (vu.hash_items(sw)[differ] != vu.hash_items(items)[differ]).all()


def test_pairing_under_given_keys():
    x, y = rows("ACGTACGT")[0], rows("TTTTACGT")[0]
    one = np.array([7, 7], np.uint64)
    assert vu.pair_under_keys(one, [x, y], one, [y, x]) == (0, 2, 0, 0, N64, N64)
    assert vu.pair_under_keys(one, [x, y], one, [x, y]) == (2, 0, 0, 0, N64, N64)
    assert vu.pair_under_keys(np.array([7, 7, 9], np.uint64), [x, x, y], np.array([7], np.uint64), [x]) == (1, 0, 2, 0, 1, N64)


def test_the_collision_seed_is_found():
    seed = vu.find_collision_seed()
    assert seed is not None and seed < 100
    u = vu.collision_salts(seed)
    assert u[0] > 0 and u[1] == 0
    r, perm = vu.collision_case(seed)
    assert np.unique(r, axis=0).shape[0] == vu.COLLISION_N and sorted(perm.tolist()) == list(range(vu.COLLISION_N))
