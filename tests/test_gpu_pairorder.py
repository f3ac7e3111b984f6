"""The pair-order coding of the paired mode that does not preserve the order, on the device (pgrc_pairorder_encode;
pgrc_amd/csrc/pairorder.hip): device == the reference-made fixtures byte for byte in every form; device ==
tests/pairorder_util's literal restatement on generator settings around the block sizes and at a million pairs, with the
input in one part and in three; at 20 M pairs device == the parallel form (which tests/test_pairorder_oracle.py ties to the
literal loop) and the literal decoder brings the device's pairs together; malformed input is PGRC_E_PARAM with the output
struct cleared and the context usable; and a paired job's reads lists, coded on the device and decoded by the literal
decoder, give the PE rows of the input reads."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import decode_util as du
import pairorder_util as po
import pgrc_amd
from pgrc_amd import PgRCDecoder, PgrcMatchError
from pgrc_amd import decode as pd
from pgrc_amd._lib import lib
from test_gpu_decode import add_lists, device_job
from test_pairorder_oracle import FIXTURES, GOLDEN, case_name, load_case

pytestmark = pytest.mark.gpu
E_PARAM = 1
MIXES = [po.DEFAULT_MIX, dict(near=0.2, jump=0.3, ret=0.15, special=0.2, drift=200, span=1 << 12),
         dict(near=0.0, jump=0.05, ret=0.02, special=0.01, drift=3, span=1 << 20)]


def assert_streams(got, want):
    form = int(want["form"])
    assert int(got["n_total"]) == int(want["n_total"]) and int(got["form"]) == form
    assert set(got) == set(want)                      # the form's streams and no others
    for k, dt in po.stream_types(form):
        assert got[k].dtype == np.dtype(dt) == np.asarray(want[k]).dtype, k
        assert got[k].size == np.asarray(want[k]).size, k
        assert got[k].tobytes() == np.asarray(want[k]).tobytes(), k


@pytest.mark.parametrize("path", FIXTURES, ids=case_name)
def test_reference_fixtures(path):
    org, st, _, _, _ = load_case(path)
    m = json.load(open(os.path.join(GOLDEN, "manifest_pairorder.json")))[case_name(path)]
    dec = PgRCDecoder(100, device=0)
    got = dec.compressReadsOrder(org, st["form"])
    assert_streams(got, st)
    t = dec.pairorder_timing()
    assert t["form"] == st["form"] and t["bytes_up"] == org.size * 4
    assert t["bytes_down"] == sum(np.asarray(st[k]).nbytes for k, _ in po.stream_types(st["form"]))
    if st["form"] != po.COMPLETE_SINGLE_FILE:         # (the single-file form codes no pair: rev alone)
        assert (t["n_near"], t["n_delta"], t["n_full"]) == (m["near"], m["delta"], m["full_set"] + m["full_keep"])
    else:
        assert (t["n_near"], t["n_delta"], t["n_full"]) == (0, 0, 0)
    assert_streams(dec.compressReadsOrder(po.split_three(org, 5), st["form"]), st)
    dec.close()
    assert_streams(pgrc_amd.compressReadsOrder(org, st["form"], device=0), st)      # a context of its own


@pytest.mark.parametrize("pairs", [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 1_000_000, 1_048_577, 2_100_000])
def test_generator_settings_equal_the_literal_loop(pairs):
    """(the device scans work in blocks of 4096 elements and carry a running fold from one round of 256 blocks to the next: 4095
    to 4097 pairs lie around one block; 1 048 577 pairs put the scans over the pairs one element past a round; at 2 100 000
    pairs, generated with next to no near pairs, the scans over the far pairs alone lie past a round too, which is asserted.
    Above a million pairs only one mix and the IGNORE form run -- a coded form that drives all four scans -- so that the
    literal loop stays at a few seconds: the other forms and mixes are not checked at these sizes.)"""
    big = pairs > 1_000_000
    dec = PgRCDecoder(100, device=0)
    for rep, knobs in enumerate([dict(po.DEFAULT_MIX, near=0.0)] if big else MIXES):
        org = po.make_order(9000 + 7 * pairs % 9973 + rep, pairs, **knobs)
        for form in (po.IGNORE,) if big else po.FORMS:
            want = po.compress_literal(org, form)
            assert pairs < 2_000_000 or np.asarray(want["delta8_flag"]).size > 1_048_576
            assert_streams(dec.compressReadsOrder(org, form), want)
            parts = po.split_three(org, pairs + rep + form)
            assert len(parts) == 3 and min(p.size for p in parts) == 0 and sum(p.size for p in parts) == org.size
            assert_streams(dec.compressReadsOrder(parts, form), want)
    dec.close()


def test_twenty_million_pairs_parallel_form_and_literal_decoder():
    pairs = 20_000_000
    org = po.make_order(2100, pairs, **po.DEFAULT_MIX)
    dec = PgRCDecoder(100, device=0)
    for form in po.FORMS:
        got = dec.compressReadsOrder(po.split_three(org, form) if form % 2 else org, form)
        assert_streams(got, po.compress_parallel(org, form))
        if form == po.IGNORE:
            k = po.kinds(got)
            assert min(k.values()) > pairs // 100, k
        if form == po.FILE_FLAGS:                     # the literal decoder on the device's streams
            order = po.decompress_literal(got)
            o = org[order]
            del order
            assert (o[0::2] % 2 == 0).all() and np.array_equal(o[1::2], o[0::2] + 1)
            assert np.array_equal(np.sort(o[0::2]), np.arange(0, 2 * pairs, 2))
    dec.close()


def _raw_encode(dec, parts, counts, form, out):
    ptrs, cnts = (pd._P * 3)(), (C.c_uint64 * 3)()
    for l in range(3):
        ptrs[l], cnts[l] = (parts[l].ctypes.data if parts[l] is not None and parts[l].size else None), counts[l]
    return lib.pgrc_pairorder_encode(dec._h, ptrs, cnts, form, C.byref(out))


def _filled():
    s = pd.PairOrderStreams()
    C.memset(C.byref(s), 0x5A, C.sizeof(s))
    return s


def test_malformed_input_is_refused_and_the_context_stays_usable():
    org = po.make_order(31, 3000)
    good = po.compress_literal(org, po.FILE_FLAGS)
    dup = org.copy()
    dup[1234] = dup[77]
    high = org.copy()
    high[2999] = org.size
    wrap = org.copy()
    wrap[5] = 0xFFFFFFFF
    empty = np.zeros(0, np.uint32)
    cases = [("odd", [org[:-1], empty, empty], None, po.FILE_FLAGS, "odd"),
             ("value >= T", [high, empty, empty], None, po.IGNORE, "or more"),
             ("value 2^32 - 1", [wrap[:3000], wrap[3000:], empty], None, po.COMPLETE, "or more"),
             ("duplicate", [dup, empty, empty], None, po.COMPLETE, "twice"),
             ("duplicate, single file", [empty, dup[:10], dup[10:]], None, po.COMPLETE_SINGLE_FILE, "twice"),
             ("unknown form", [org, empty, empty], None, 4, "form"),
             ("negative form", [org, empty, empty], None, -1, "form"),
             ("2^32 entries", [org, empty, empty], [1 << 32, 0, 0], po.IGNORE, "2^32"),
             ("2^32 entries in all", [org, org, empty], [1 << 31, 1 << 31, 0], po.IGNORE, "2^32"),
             ("NULL list", [org, None, empty], [org.size, 2, 0], po.IGNORE, "NULL")]
    dec = PgRCDecoder(100, device=0)
    for what, parts, counts, form, names in cases:
        out = _filled()
        rc = _raw_encode(dec, parts, counts or [0 if p is None else p.size for p in parts], form, out)
        msg = (lib.pgrc_decode_last_error(dec._h) or b"").decode()
        assert rc == E_PARAM and names in msg, (what, rc, msg)
        assert bytes(out) == bytes(C.sizeof(out)), what                # *out is cleared
        # ... and the same context codes a good order right away
        got = dec.compressReadsOrder(org, po.FILE_FLAGS)
        assert_streams(got, good)
    with pytest.raises(PgrcMatchError) as e:                               # the wrapper raises the same
        dec.compressReadsOrder(dup, po.FILE_FLAGS)
    assert e.value.code == E_PARAM and "twice" in str(e.value)
    assert lib.pgrc_pairorder_encode(dec._h, None, None, 0, None) == E_PARAM
    dec.close()
    fresh = PgRCDecoder(100, device=0)
    with pytest.raises(PgrcMatchError) as e:
        fresh.pairorder_timing()
    assert e.value.code == 6
    fresh.close()


def test_paired_job_order_through_the_literal_decoder_gives_the_pe_rows():
    L = 100
    case, res, pg_st, org_st = device_job(733, L, True)
    dc = du.decode_case(case, res, pg_st, org_st, pair=True)
    rl = dc["rl_idx_order"]                          # rlIdx of every original index: the encoder's rev
    T = rl.size
    org = np.empty(T, np.uint32)
    org[rl] = np.arange(T, dtype=np.uint32)
    n = [lst["n"] for lst in dc["lists"]]
    assert sum(n) == T and min(n) > 0
    parts = [org[:n[0]], org[n[0]:n[0] + n[1]], org[n[0] + n[1]:]]     # the three reads lists' orgIdx arrays
    dec = PgRCDecoder(L, device=0)
    dec.set_text(dc["text"])
    add_lists(dec, dc["lists"])
    want1, want2 = dec.writeAllReadsInPEMode(rl, revComplPairFile=True)
    for p, w in enumerate((want1, want2)):
        assert np.array_equal(w, du.truth_rows_pe(dc, p)), p
    # COMPLETE: the decoded order is the case's rlIdxOrder itself
    st = dec.compressReadsOrder(parts, po.COMPLETE)
    assert_streams(st, po.compress_literal(org, po.COMPLETE))
    order = po.decompress_literal(st)
    assert np.array_equal(order, rl)
    f1, f2 = dec.writeAllReadsInPEMode(order, revComplPairFile=True)
    assert np.array_equal(f1, want1) and np.array_equal(f2, want2)
    assert np.array_equal(dec.compressReadsOrder(parts, po.COMPLETE_SINGLE_FILE)["rev"], rl)
    # FILE_FLAGS: the pairs in another order, every row pair still one original pair, file 1 the even read
    st = dec.compressReadsOrder(parts, po.FILE_FLAGS)
    order = po.decompress_literal(st)
    assert not np.array_equal(order, rl)
    f1, f2 = dec.writeAllReadsInPEMode(order, revComplPairFile=True)
    o = org[order].astype(np.int64)
    q = o[0::2] // 2                                  # the original pair of every row
    assert np.array_equal(o[0::2], 2 * q) and np.array_equal(o[1::2], 2 * q + 1)
    assert np.array_equal(np.sort(q), np.arange(T // 2))                  # every pair once
    assert np.array_equal(f1, want1[q]) and np.array_equal(f2, want2[q])
    assert np.array_equal(f1, du.truth_rows_pe(dc, 0)[q]) and np.array_equal(f2, du.truth_rows_pe(dc, 1)[q])
    k = po.kinds(st)
    assert k["near"] > 0 and k["delta"] + k["full_set"] + k["full_keep"] > 0, k
    dec.close()
