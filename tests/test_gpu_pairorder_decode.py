"""The pair-order decoder on the device (pgrc_pairorder_decode, pgrc_decode_set_order_pair_order_streams;
pgrc_amd/csrc/pairorder.hip): device == the reference-made fixtures' decoded orders byte for byte in every
form; device == tests/pairorder_util's literal loop on generated orders -- sizes around a word, the all-adjacent order,
constant offsets around a word and around the near / far limit, the nested and the halves order, and offsets around the
reach of the landing's ring with the real batch size; encoder -> decoder round trips in all four forms; a PE job's rows
from the streams equal the rows from the decoded array; every refusal is PGRC_E_PARAM with its message, the output
untouched and the context usable; the landing's word and round counts are the restatement's."""
import ctypes as C

import numpy as np
import pytest

import decode_util as du
import pairorder_decode_util as pdu
import pairorder_util as po
import pgrc_amd
from pgrc_amd import PgRCDecoder, PgrcMatchError
from pgrc_amd import decode as pd
from pgrc_amd._lib import lib
from test_gpu_decode import add_lists
from test_pairorder_oracle import FIXTURES, case_name, load_case

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = 1, 6
ORDERS = pdu.generated_orders(pdu.BATCH)
_LITERAL = {}


def literal(name, org, form):
    """(the literal encoder's streams, the literal decoder's order) of a generated order, made once"""
    if (name, form) not in _LITERAL:
        st = po.compress_literal(org, form)
        _LITERAL[name, form] = (st, po.decompress_literal(st))
    return _LITERAL[name, form]


@pytest.fixture(scope="module")
def dec():
    d = PgRCDecoder(100, device=0)
    yield d
    d.close()


@pytest.mark.parametrize("path", FIXTURES, ids=case_name)
def test_reference_fixtures(dec, path):
    _, st, decoded, _, _ = load_case(path)
    got = dec.decompressReadsOrder(st)
    assert got.dtype == decoded.dtype and got.tobytes() == decoded.tobytes()
    t = dec.pairorder_decode_timing()
    assert t["form"] == st["form"] and t["bytes_down"] == decoded.nbytes
    assert t["bytes_up"] == sum(np.asarray(st[k]).nbytes for k, _ in po.stream_types(st["form"]))
    if st["form"] != po.COMPLETE_SINGLE_FILE:
        k = po.kinds(st)
        assert (t["n_near"], t["n_delta"], t["n_full"]) == (k["near"], k["delta"], k["full_set"] + k["full_keep"])
    assert np.array_equal(pgrc_amd.decompressReadsOrder(st, ctx=dec), decoded)
    assert np.array_equal(pgrc_amd.decompressReadsOrder(st, device=0), decoded)             # a context of its own


@pytest.mark.parametrize("name,org", ORDERS, ids=[n for n, _ in ORDERS])
def test_generated_orders_equal_the_literal_loop(dec, name, org):
    for form in po.FORMS:
        st, want = literal(name, org, form)
        got = dec.decompressReadsOrder(st)
        assert got.dtype == np.uint32 and got.tobytes() == want.tobytes(), (name, form)


def test_the_batch_order_reaches_the_bitmap_with_the_real_batch():
    name, org = ORDERS[-1]
    assert name == "batches" and org.size == 12 * pd.PGRC_PAIRORDER_DECODE_BATCH
    d, _, _ = pdu.offsets(literal(name, org, po.IGNORE)[0])
    B = pd.PGRC_PAIRORDER_DECODE_BATCH
    assert {3 * B - 1, 3 * B, 3 * B + 1, 4 * B + 5} <= set(d.tolist())
    bases = literal(name, org, po.IGNORE)[1][0::2]
    assert np.unique(bases[d >= 3 * B] // B).size >= 4                     # marks into the bitmap from several batches


@pytest.mark.parametrize("pairs", [1, 64, 4097, 70_000])
def test_round_trip_with_the_encoder(dec, pairs):
    org = np.random.default_rng(600 + pairs).permutation(2 * pairs).astype(np.uint32)
    rev = np.empty(org.size, np.uint32)
    rev[org] = np.arange(org.size, dtype=np.uint32)
    for form in po.FORMS:
        out = dec.decompressReadsOrder(dec.compressReadsOrder(po.split_three(org, pairs + form), form))
        if form in (po.COMPLETE, po.COMPLETE_SINGLE_FILE):
            assert np.array_equal(out, rev), form
        elif form == po.FILE_FLAGS:
            o = org[out]
            assert (o[0::2] % 2 == 0).all() and np.array_equal(o[1::2], o[0::2] ^ 1)
            assert np.unique(o).size == o.size
        else:
            assert po.pairs_are_mates(out, org) and (out[0::2] < out[1::2]).all()
            assert (np.diff(out[0::2].astype(np.int64)) > 0).all()


def _job(seed=11, L=40):
    """three small lists by hand: an HQ list with RC flags and mismatches, an LQ and an N list"""
    rng = np.random.default_rng(seed)
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=30_000)].copy()
    n = 300
    cnt = rng.integers(0, 3, n).astype(np.uint8)
    offs = np.concatenate([np.sort(rng.choice(L, size=c, replace=False)) for c in cnt]).astype(np.int64)
    hq = {"text_base": 0, "n": n, "off": rng.integers(0, 60, n).astype(np.uint8), "rc": (rng.random(n) < 0.5).astype(np.uint8),
          "mis_cnt": cnt, "mis_sym": rng.integers(0, 4, offs.size).astype(np.uint8),
          "mis_off": du.offsets_to_rev_offsets(cnt, offs, L).astype(np.uint8), "rev_coded": True, "form": 0, "order": b"TGNAC"}
    lq = {"text_base": 20_000, "n": 70, "off": rng.integers(0, 50, 70).astype(np.uint8)}
    nl = {"text_base": 25_000, "n": 30, "pos": np.arange(30) * 9}
    return {"L": L, "text": text, "lists": [hq, lq, nl]}, n + 100


@pytest.mark.parametrize("pair_file", [False, True])
def test_job_order_from_the_streams_gives_the_rows_of_the_decoded_array(pair_file):
    dc, T = _job()
    org = po.make_order(808, T // 2)
    d = PgRCDecoder(dc["L"], device=0)
    d.set_text(dc["text"])
    add_lists(d, dc["lists"])
    for form in po.FORMS:
        st = po.compress_literal(org, form)
        order = d.decompressReadsOrder(st)
        assert np.array_equal(order, po.decompress_literal(st))
        want = d.writeAllReadsInPEMode(order, revComplPairFile=pair_file)
        for p, w in enumerate(du.write_pe(dc, order, pair_file)):
            assert np.array_equal(want[p], w), (form, p)
        d.set_order(pd.PGRC_DECODE_SE)                                      # (another order in between)
        d.set_order_pair_order_streams(st, pair_file)
        assert d.row_count(0) == d.row_count(1) == T // 2
        for p in range(2):
            assert np.array_equal(d.rows(p), want[p]), (form, p)
        t = d.pairorder_decode_timing()
        assert t["form"] == form and t["bytes_down"] == 0 and t["ms_download"] == 0
    # an order of more entries than the lists hold, and an index beyond them: refused, and no order is left
    for bad, names in ((po.compress_literal(po.make_order(5, T // 2 + 1), po.IGNORE), "n_total differs"),
                       (dict(po.compress_literal(org, po.COMPLETE_SINGLE_FILE), rev=np.where(np.arange(T) == 7, T, org).astype(np.uint32)), "out of range"),
                       (pdu.near_streams([2, 1] + [1] * (T // 2 - 2)), "pair order (decode)")):
        d.set_order_pair_order_streams(po.compress_literal(org, po.IGNORE), pair_file)
        assert d.row_count(0) == T // 2
        with pytest.raises(PgrcMatchError) as e:
            d.set_order_pair_order_streams(bad, pair_file)
        assert e.value.code == E_PARAM and names in str(e.value), str(e.value)
        with pytest.raises(PgrcMatchError) as e:
            d.row_count(0)
        assert e.value.code == E_STATE
    d.close()


CASES = pdu.refusal_cases()


@pytest.mark.parametrize("what,st,names", CASES, ids=[c[0] for c in CASES])
def test_refusals(dec, what, st, names):
    good_org = po.make_order(32, 700)
    good = po.compress_literal(good_org, po.FILE_FLAGS)
    s, keep = pd._pairorder_struct(st)
    n = min(int(st["n_total"]), 1 << 16)
    out = np.full(n + 8, 0xA5A5A5A5, np.uint32)
    rc = lib.pgrc_pairorder_decode(dec._h, C.byref(s), out.ctypes.data_as(pd._P))
    msg = (lib.pgrc_decode_last_error(dec._h) or b"").decode()
    assert rc == E_PARAM and names in msg and "pair order (decode)" in msg, (what, rc, msg)
    assert (out == 0xA5A5A5A5).all(), what                                 # rl_idx_order is untouched
    if int(st["n_total"]) < 1 << 24:                                        # (the wrapper allocates the output)
        with pytest.raises(PgrcMatchError) as e:                            # the wrapper raises the same
            dec.decompressReadsOrder(st)
        assert e.value.code == E_PARAM and names in str(e.value)
    # ... and the same context decodes a good order right away
    assert np.array_equal(dec.decompressReadsOrder(good), po.decompress_literal(good))


def test_null_arguments_and_timing_state():
    d = PgRCDecoder(100, device=0)
    with pytest.raises(PgrcMatchError) as e:
        d.pairorder_decode_timing()
    assert e.value.code == E_STATE
    st = po.compress_literal(po.make_order(1, 10), po.IGNORE)
    s, keep = pd._pairorder_struct(st)
    assert lib.pgrc_pairorder_decode(d._h, None, None) == E_PARAM
    assert lib.pgrc_pairorder_decode(d._h, C.byref(s), None) == E_PARAM and "rl_idx_order is NULL" in lib.pgrc_decode_last_error(d._h).decode()
    s.struct_size -= 4
    assert lib.pgrc_pairorder_decode(d._h, C.byref(s), None) == E_PARAM and "struct_size" in lib.pgrc_decode_last_error(d._h).decode()
    with pytest.raises(PgrcMatchError) as e:                                # no list: no PE order
        d.set_order_pair_order_streams(st)
    assert e.value.code == E_STATE
    empty = dict(st, n_total=0, **{k: np.zeros(0, dt) for k, dt in po.stream_types(po.IGNORE)})
    assert d.decompressReadsOrder(empty).size == 0
    t = pd.PairOrderDecodeTiming()
    assert lib.pgrc_pairorder_get_decode_timing(d._h, C.byref(t)) == E_PARAM               # struct_size is not set
    d.close()


def test_landing_counts(dec):
    """landing_words is the words swept; a word whose offsets all leave it takes one round; the all-adjacent order takes a
    round per pair of a word and one more (the restatement's count, which the device's equals on every small order)"""
    for dd in (64, 65, 255, 256):
        org = pdu.constant_offset_order(dd, 3, dd)
        dec.decompressReadsOrder(po.compress_literal(org, po.IGNORE))
        t = dec.pairorder_decode_timing()
        # the sweep ends with the last base, in the first half of the last block of 2 * dd slots
        assert t["landing_words"] == -(-(2 * dd * 2 + dd) // 64) and t["landing_rounds"] == t["landing_words"], (dd, t)
    pairs = 4096
    dec.decompressReadsOrder(po.compress_literal(pdu.adjacent_order(pairs), po.IGNORE))
    t = dec.pairorder_decode_timing()
    assert t["landing_words"] == 2 * pairs // 64
    assert 31 * t["landing_words"] <= t["landing_rounds"] <= 34 * t["landing_words"], t     # about 32 a word: 32 pairs and the last look
    for name, org in ORDERS[:-1]:
        stats = {}
        pdu.decode(literal(name, org, po.IGNORE)[0], pdu.BATCH, stats)
        dec.decompressReadsOrder(literal(name, org, po.IGNORE)[0])
        t = dec.pairorder_decode_timing()
        assert (t["landing_words"], t["landing_rounds"]) == (stats["landing_words"], stats["landing_rounds"]), name
        last_base = int(literal(name, org, po.IGNORE)[1][-2])
        assert t["landing_words"] == last_base // 64 + 1, name              # ceil(slots swept / 64)
