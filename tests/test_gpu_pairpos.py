"""The pair-position coding of the order-preserving paired mode on the device (pgrc_pairpos_encode / _decode,
pgrc_decode_set_order_pair_streams; pgrc_amd/csrc/pairpos.hip): device == the reference-made fixtures byte for byte in
both directions; device == tests/pairpos_util's literal restatement on random generator settings around the sort's tile
and up to a million pairs, both position widths, and at 20 M pairs a device round trip plus streams equal to the
three-state form (which tests/test_pairpos_oracle.py ties to the literal loop); malformed input is PGRC_E_PARAM and
leaves the context without an order; and a paired ORD job decodes to the same rows from the streams as from the host
array, also after the restore of the matched pseudogenomes on the same context."""
import os

import numpy as np
import pytest

import decode_util as du
import pairpos_util as pp
import pgmap_util as pu
import pgrc_amd
from pgrc_amd import PgRCDecoder, PgrcMatchError
from pgrc_amd.decode import PGRC_DECODE_ORD
from test_gpu_decode import add_lists, device_job
from test_gpu_restore import device_matches
from test_pairpos_oracle import FIXTURES, load_case

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = 1, 6


def counts_of(st):
    return [int(np.asarray(st[k]).size) for k in ("off_value", "delta16_flag", "delta_value", "not_base_pos")]


def assert_streams(got, want):
    assert int(got["n_total"]) == int(want["n_total"]) and int(got["pos_width"]) == int(want["pos_width"])
    assert counts_of(got) == counts_of(want)
    for k in pp.STREAMS:
        assert got[k].dtype == np.asarray(want[k]).dtype, k
        assert got[k].tobytes() == np.asarray(want[k]).tobytes(), k


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def test_reference_fixtures_both_directions(path):
    org, st, decoded, _ = load_case(path)
    dec = PgRCDecoder(100, device=0)
    got = dec.compressReadsPgPositions(org, st["pos_width"])
    assert_streams(got, st)
    t = dec.pairpos_timing()
    k = pp.kinds(st)
    assert (t["encode"], t["n_near"], t["n_delta"], t["n_full"]) == (1, k["near"], k["delta"], k["full_set"] + k["full_keep"])
    back = dec.decompressReadsPgPositions(st)
    assert back.dtype == np.uint64 and back.tobytes() == decoded.tobytes()
    assert dec.pairpos_timing()["encode"] == 0
    dec.close()
    # the module-level forms (a context of their own)
    assert_streams(pgrc_amd.compressReadsPgPositions(org, st["pos_width"], device=0), st)
    assert np.array_equal(pgrc_amd.decompressReadsPgPositions(st, device=0), decoded)


@pytest.mark.parametrize("W", [4, 8])
@pytest.mark.parametrize("pairs", [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 1_000_000, 1_048_577, 2_100_000])
def test_random_settings_equal_the_restatement(pairs, W):
    """(the device scans work in blocks of 4096 elements and carry a running fold from one round of 256 blocks to the next: 4095
    to 4097 pairs lie around one block; 1 048 577 pairs put the scans over the pairs one element past a round; at 2 100 000
    pairs, generated without near pairs, the scans over the far pairs alone lie past a round too, which is asserted)"""
    dec = PgRCDecoder(100, device=0)
    for rep in range(3 if pairs < 100_000 else 1):
        seed = 7000 + 10 * pairs % 9973 + 3 * rep + W
        knobs = [pp.DEFAULT_MIX, dict(near=0.2, jump=0.3, ret=0.15, tie=0.3, special=0.2),
                 dict(near=0.0, jump=0.05, ret=0.02, tie=0.0, special=0.01, drift=30000)][rep]
        if pairs > 1_000_000:
            knobs = dict(pp.DEFAULT_MIX, near=0.0)
        org = pp.make_positions(seed, pairs, W, **knobs)
        want = pp.compress_literal(org, W)
        assert pairs < 2_000_000 or np.asarray(want["delta16_flag"]).size > 1_048_576
        got = dec.compressReadsPgPositions(org, W)
        assert_streams(got, want)
        assert np.array_equal(dec.decompressReadsPgPositions(want), pp.decompress_literal(want))
    dec.close()


@pytest.mark.parametrize("W", [4, 8])
def test_twenty_million_pairs_round_trip_and_three_state_streams(W):
    pairs = 20_000_000
    org = pp.make_positions(2000 + W, pairs, W, **pp.DEFAULT_MIX)
    dec = PgRCDecoder(100, device=0)
    got = dec.compressReadsPgPositions(org, W)
    back = dec.decompressReadsPgPositions(got)
    dec.close()
    assert np.array_equal(back, pp.file_major(org))
    want = pp.compress_states(org, W)
    assert_streams(got, want)
    k = pp.kinds(got)
    assert min(k.values()) > pairs // 100, k


def test_non_unit_flags_follow_the_reference():
    """the reference reads `offsetInUint16Flag[i] == 1` and `if (deltaInInt16Flag[..])`: other flag bytes mean far / delta"""
    org = pp.make_positions(5, 3000, 4, **pp.DEFAULT_MIX)
    st = pp.compress_literal(org, 4)
    st["off16_flag"] = np.where(st["off16_flag"] == 0, 2, 1).astype(np.uint8)
    st["delta16_flag"] = (st["delta16_flag"] * 7).astype(np.uint8)
    dec = PgRCDecoder(100, device=0)
    assert np.array_equal(dec.decompressReadsPgPositions(st), pp.file_major(org))
    dec.close()


def _ord_job(L=100, seed=611):
    case, res, pg_st, org_st = device_job(seed, L, True)
    dc = du.decode_case(case, res, pg_st, org_st, pair=True)
    return dc


def _tamper(st, what):
    st = dict(st)
    if what == "odd n_total":
        st["n_total"] = st["n_total"] - 1
    elif what == "pos_width":
        st["pos_width"] = 2
        st["base_pos"], st["not_base_pos"] = st["base_pos"].astype(np.uint32), st["not_base_pos"].astype(np.uint32)
    elif what == "NULL":
        st["n_off16"] = st["off_value"].size
        st["off_value"] = np.zeros(0, np.uint16)
    elif what == "n_off16":
        st["off_value"], st["off_base_first"] = st["off_value"][:-1], st["off_base_first"][:-1]
    elif what == "n_delta_flag":
        st["delta16_flag"] = np.concatenate([st["delta16_flag"], np.zeros(1, np.uint8)])
        st["not_base_pos"] = np.concatenate([st["not_base_pos"], st["not_base_pos"][:1]])
    elif what == "n_delta16":
        st["delta_value"], st["delta_base_first"] = st["delta_value"][:-1], st["delta_base_first"][:-1]
    elif what == "n_not_base":
        st["not_base_pos"] = st["not_base_pos"][:-1]
    return st


MALFORMED = [("odd n_total", "n_total is odd"), ("pos_width", "pos_width"), ("NULL", "NULL"), ("n_off16", "n_off16"),
             ("n_delta_flag", "n_delta_flag"), ("n_delta16", "n_delta16"), ("n_not_base", "n_not_base")]


def test_malformed_streams_are_refused_and_leave_no_order():
    dc = _ord_job()
    o2p = dc["org2pos"]
    good = pp.compress_literal(pp.interleaved(o2p), 4)
    dec = PgRCDecoder(dc["L"], device=0)
    dec.set_text(dc["text"])
    add_lists(dec, dc["ord_lists"])
    for what, names in MALFORMED:
        dec.set_order(PGRC_DECODE_ORD, o2p.size, org_idx_to_pos=o2p, paired=True)
        assert dec.row_count(0) == o2p.size // 2
        bad = _tamper(good, what)
        with pytest.raises(PgrcMatchError) as e:
            dec.set_order_pair_streams(bad)
        assert e.value.code == E_PARAM and names in str(e.value), (what, str(e.value))
        with pytest.raises(PgrcMatchError) as e:
            dec.row_count(0)
        assert e.value.code == E_STATE, what
        with pytest.raises(PgrcMatchError) as e:          # the same to the host
            dec.decompressReadsPgPositions(bad)
        assert e.value.code == E_PARAM and names in str(e.value), (what, str(e.value))
    # a position past the text end: set_order's own check, on the decoded positions
    far = o2p.copy()
    far[3] = dc["text"].size - dc["L"] + 1
    with pytest.raises(PgrcMatchError) as e:
        dec.set_order_pair_streams(pp.compress_literal(pp.interleaved(far), 4))
    assert e.value.code == E_PARAM and "window" in str(e.value)
    with pytest.raises(PgrcMatchError) as e:
        dec.row_count(0)
    assert e.value.code == E_STATE
    # the encoder's refusals
    for org, W, names in ((np.zeros(3, np.uint64), 4, "n_total is odd"), (np.zeros(4, np.uint64), 5, "pos_width"),
                          (np.array([5, 1 << 32, 7, 9], np.uint64), 4, "2^32"), (np.array([1 << 32, 5, 7, 9], np.uint64), 4, "2^32")):
        with pytest.raises(PgrcMatchError) as e:
            dec.compressReadsPgPositions(org, W)
        assert e.value.code == E_PARAM and names in str(e.value), str(e.value)
    # and the same context takes well-formed streams afterwards
    dec.set_order_pair_streams(good, rev_compl_pair_file=True)
    assert dec.row_count(1) == o2p.size // 2
    dec.close()


def test_paired_ord_job_from_streams_equals_the_host_array_and_the_reads():
    dc = _ord_job()
    L, o2p = dc["L"], dc["org2pos"]
    text = dc["text"].copy()
    a, b = PgRCDecoder(L, device=0), PgRCDecoder(L, device=0)
    a.set_text(text)
    add_lists(a, dc["ord_lists"])
    st = a.compressReadsPgPositions(pp.interleaved(o2p), 4)                 # orgIdx2PgPos encoded on the device
    assert_streams(st, pp.compress_literal(pp.interleaved(o2p), 4))
    b.set_text(text)
    add_lists(b, dc["ord_lists"])
    for rcpf in (False, True):
        a.set_order_pair_streams(st, rev_compl_pair_file=rcpf)
        b.set_order(PGRC_DECODE_ORD, o2p.size, org_idx_to_pos=o2p, paired=True, rev_compl_pair_file=rcpf)
        for p in range(2):
            assert a.row_count(p) == b.row_count(p) == o2p.size // 2
            got = a.rows(p)
            assert np.array_equal(got, b.rows(p)), (rcpf, p)
            if rcpf:                                                         # (the job was made with the pair-file rule)
                assert np.array_equal(got, du.truth_rows_ord(dc, text, p, True)), p
    # once more with the text restored on the device: restore -> order -> rows on one context
    hq_len = dc["lists"][1]["text_base"]
    lq_len = dc["lists"][2]["text_base"] - hq_len
    rng = np.random.default_rng(L)
    for _ in range(60):
        ln = int(rng.integers(50, 400))
        s, d = int(rng.integers(0, hq_len - ln)), int(rng.integers(0, text.size - ln))
        text[d:d + ln] = pu.revcomp_np(text[s:s + ln])
    hq, lq, nn = text[:hq_len], text[hq_len:hq_len + lq_len], text[hq_len + lq_len:]
    mapped, lens, offs, lns, found = pu.map_all(hq, lq, nn, device_matches(hq, 36), 36)
    assert found[0].shape[0] > 0
    a.restoreMatchedPgs(mapped, lens, hq.size, offs, lns)
    with pytest.raises(PgrcMatchError) as e:                                 # (the lists and the order were dropped)
        a.set_order_pair_streams(st, rev_compl_pair_file=True)
    assert e.value.code == E_STATE
    add_lists(a, dc["ord_lists"])
    a.set_order_pair_streams(st, rev_compl_pair_file=True)
    b.set_text(text)
    add_lists(b, dc["ord_lists"])
    b.set_order(PGRC_DECODE_ORD, o2p.size, org_idx_to_pos=o2p, paired=True, rev_compl_pair_file=True)
    for p in range(2):
        assert np.array_equal(a.rows(p), b.rows(p)), p
    t = a.pairpos_timing()
    assert t["encode"] == 0 and t["bytes_down"] == 0 and t["bytes_up"] < o2p.size * 8
    a.close()
    b.close()
