"""The two rules tests/test_gpu_rlist_ord.py leans on, pinned without a GPU.

The narrowing of orgIdx2PgPos in the single-file order-preserving mode, restated from compressReadsPgPositions
(SeparatedPseudoGenomePersistence.cpp:454-459: with singleFileMode every element of the vector of eight-byte positions is stored
as `(uint_pg_len) orgIdx2PgPos[i]` from the start of the same buffer, so the first T * sizeof(uint_pg_len) bytes are what is
written), against rlist_util.positions_numpy on the seeded settings; and export_util.original_order_entries against the org_idx
streams of the committed "org" fixtures, which are the reference's own bytes."""
import numpy as np
import pytest

import export_util as xu
import rlist_util as rl


def narrow_literal(positions, width):
    """:454-459 line by line: PgPosPtr walks the vector's own storage in steps of `width` bytes; element i is read before the
    place it is written to can reach it (the write pointer never overtakes the read index) -> the bytes handed to writeCompressed"""
    buf = bytearray(np.asarray(positions, dtype="<u8").tobytes())
    T = len(buf) // 8
    if width < 8:
        for i in range(T):
            v = int.from_bytes(buf[8 * i: 8 * i + 8], "little")
            buf[width * i: width * i + width] = (v & ((1 << (8 * width)) - 1)).to_bytes(width, "little")
    return bytes(buf[: T * width])


def narrow_numpy(positions, width):
    """what ReadsList.positions returns: the positions as uint32 / uint64"""
    return np.asarray(positions, dtype=np.uint64).astype(np.uint32 if width == 4 else np.uint64)


SETTINGS = [(seed, None) for seed in range(8)] + [(11, 1), (12, 3), (13, 2999)]


@pytest.mark.parametrize("seed,T", SETTINGS)
def test_narrowing_of_the_seeded_settings(seed, T):
    s = rl.make_setting(seed, T=T)
    arr = rl.positions_of(s, rl.positions_numpy)
    assert np.array_equal(arr, rl.positions_of(s, rl.positions_literal)) and arr.size == s["T"]
    assert (rl.writers_per_index(s["T"], s["hq"], s["lq"], s["n"], s["read_org"], s["match_pos"]) == 1).all()
    for W in (4, 8):
        got = narrow_numpy(arr, W)
        assert got.dtype.itemsize == W and got.tobytes() == narrow_literal(arr, W)
        if W == 8 or int(arr.max(initial=0)) < 2**32:
            assert np.array_equal(got.astype(np.uint64), arr)           # nothing is lost where every position fits
    if T is not None:
        assert s["T"] == T and T % 2 == 1                               # the odd totals the paired call refuses


def test_some_seeded_setting_crosses_four_bytes():
    """the W = 4 refusal of the GPU test needs a setting with a position of 2^32 or more, and the equality one without"""
    tops = [int(rl.positions_of(rl.make_setting(seed), rl.positions_numpy).max(initial=0)) for seed in range(8)]
    assert any(t >= 2**32 for t in tops) and any(t < 2**32 for t in tops)


@pytest.mark.parametrize("name", xu.EXPORT_GOLDEN)
def test_entry_rule_equals_the_fixtures(name):
    case, pair, kmax, res, order, gold = xu.load_export_golden(name)
    n = case["reads"].shape[0]
    matched = res["mism"] != 255
    er, eo = xu.original_order_entries(case["read_org"], matched, case["total"], pair, n - case["n_n"])
    assert eo.tobytes() == gold["org"]["org_idx"]
    # one entry per index that no unmatched read carries; a filler exactly where no read of the matcher carries the index
    assert er.size == case["total"] - int((~matched).sum())
    fill = er == 0xFFFFFFFF
    assert not np.isin(eo[fill], case["read_org"]).any() and np.array_equal(case["read_org"][er[~fill]], eo[~fill])
    if pair:
        k = int((eo % 2 == 0).sum())
        assert (eo[:k] % 2 == 0).all() and (eo[k:] % 2 == 1).all() and (np.diff(eo[:k].astype(np.int64)) > 0).all() and (np.diff(eo[k:].astype(np.int64)) > 0).all()
    else:
        assert (np.diff(eo.astype(np.int64)) > 0).all()
