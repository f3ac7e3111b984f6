"""The archive form of a reads list's mismatch streams on the device (pgrc_list_archive_encode, pgrc_decode_add_list_archive;
pgrc_amd/csrc/listarchive.hip): device == the reference-made fixtures byte for byte in both directions; encode == the literal
loops of tests/listarchive_util on generator settings around the scan block (4096), the split's tile (8192) and past one carry
round of the scans (1 048 577), in three count mixes and at both coder levels, and the lists rebuilt from the device's own
streams give the rows pgrc_decode_add_list gives with the original streams; entries of 254 mismatches at L = 255; a matched
and exported job through encode and add_list_archive gives the input reads; every refusal leaves the output cleared (encode),
no list added (decode) and the context usable."""
import ctypes as C

import numpy as np
import pytest

import decode_util as du
import listarchive_util as la
from pgrc_amd import PgRCDecoder, PgrcMatchError
from pgrc_amd import decode as pd
from pgrc_amd._lib import ExportStreams, ListArchiveStreams, lib
from test_gpu_decode import add_lists, device_job

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = 1, 6
TILE = pd.PGRC_LIST_ARCHIVE_TILE
MIXES = {"mostly_zero": dict(zero=0.95, counts=(1, 2, 3, 4, 6), weights=(8, 4, 2, 1, 1)),
         "no_zero": dict(zero=0.0, counts=(1, 2, 3), weights=(3, 2, 1)),
         "one_count": dict(zero=0.3, counts=(2,))}
SIZES = [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, TILE - 1, TILE, TILE + 1, 1_048_577]


def text_for(n, L, seed=5):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, size=n + L)]


def rows_plain(L, text, cnt, codes, order, off, rev_coded):
    dec = PgRCDecoder(L, device=0)
    dec.set_text(text)
    dec.add_list(cnt.size, 0, pos=np.arange(cnt.size, dtype=np.uint64), rev_comp=(np.arange(cnt.size) % 3 == 0).astype(np.uint8), mis_cnt=cnt,
                 mis_sym=codes, mis_off=off, mis_off_rev_coded=rev_coded, mis_sym_form=0, bases_order=order)
    rows = dec.writeAllReadsInSEMode()
    dec.close()
    return rows


def rows_archive(L, text, st, dec=None):
    own = dec is None
    if own:
        dec = PgRCDecoder(L, device=0)
    n = int(st["n_entries"])
    dec.set_text(text)
    dec.add_list_archive(n, st, 0, pos=np.arange(n, dtype=np.uint64), rev_comp=(np.arange(n) % 3 == 0).astype(np.uint8))
    rows = dec.writeAllReadsInSEMode()
    t = dec.list_archive_timing()
    assert t["encode"] == 0 and t["n_nonzero"] == int(st["n_nonzero"]) and t["limit"] == int(np.asarray(st["props"])[0])
    if own:
        dec.close()
    return rows


@pytest.mark.parametrize("path", la.fixtures(), ids=la.case_name)
def test_reference_fixtures_both_directions(path):
    L, fast, (cnt, sym, off, rev_off), st, (lcnt, lsym, loff) = la.load_case(path)
    dec = PgRCDecoder(L, device=0)
    got = dec.list_archive_encode(cnt, sym, rev_off, fast)
    la.assert_streams(got, st)
    assert got["one_block"]
    t = dec.list_archive_timing()
    assert t["encode"] == 1 and t["bytes_up"] == cnt.size + 2 * sym.size and t["limit"] == int(st["props"][0])
    assert t["n_nonzero"] == st["n_nonzero"] and t["bytes_down"] >= cnt.size + st["n_nonzero"] + 2 * sym.size
    # the loader's side: the reference's streams rebuilt on the device == its loaded list through pgrc_decode_add_list
    text = text_for(cnt.size, L)
    want = rows_plain(L, text, lcnt, lsym, st["bases_order"], loff, False)
    assert np.array_equal(rows_archive(L, text, st, dec), want)
    assert np.array_equal(rows_archive(L, text, got), want)
    dec.close()


@pytest.mark.parametrize("mix", list(MIXES))
@pytest.mark.parametrize("n", SIZES)
def test_generator_settings_equal_the_literal_loops(n, mix):
    """(the scans work in blocks of 4096 elements and carry a fold from one round of 256 blocks to the next; the split works in
    tiles of 8192 entries.  Past 10 000 entries the rebuilt rows are compared for one mix only.)"""
    L = 40
    cnt, sym, rev_off = la.make_list(7000 + n % 977, n, L, **MIXES[mix])
    want = la.encode_literal(cnt, sym, rev_off, False)
    dec = PgRCDecoder(L, device=0)
    got = dec.list_archive_encode(cnt, sym, rev_off, False)
    la.assert_streams(got, want)
    props, dests = la.split_offsets_literal(cnt, rev_off, True)
    fast = dec.list_archive_encode(cnt, sym, rev_off, True)
    la.assert_streams(fast, dict(want, props=props, dests=dests))
    if n <= 10_000 or mix == "no_zero":
        text = text_for(n, L)
        rows = rows_plain(L, text, cnt, want["mis_sym"], want["bases_order"], rev_off, True)
        assert np.array_equal(rows_archive(L, text, got, dec), rows)
        if n <= 10_000:
            assert np.array_equal(rows_archive(L, text, fast, dec), rows)
    dec.close()


def test_entries_of_254_mismatches():
    L = 255
    cnt, sym, rev_off = la.make_list(81, 300, L, zero=0.0, counts=(254,))
    want = la.encode_literal(cnt, sym, rev_off, False)
    assert int(want["props"][0]) == 254 and want["dests"][254].size == 300 * 254
    dec = PgRCDecoder(L, device=0)
    got = dec.list_archive_encode(cnt, sym, rev_off, False)
    la.assert_streams(got, want)
    text = text_for(300, L)
    assert np.array_equal(rows_archive(L, text, got, dec), rows_plain(L, text, cnt, want["mis_sym"], want["bases_order"], rev_off, True))
    dec.close()


def test_a_device_job_through_both_calls_gives_the_reads():
    L = 100
    case, res, pg_st, _ = device_job(733, L, False)
    dc = du.decode_case(case, res, pg_st)
    hq = dc["lists"][0]
    assert pg_st["mis_cnt"].sum() > 100 and (pg_st["mis_cnt"] == 0).sum() > 100
    dec = PgRCDecoder(L, device=0)
    st = dec.list_archive_encode(pg_st["mis_cnt"], pg_st["mis_sym"], pg_st["mis_rev_off"])
    la.assert_streams(st, la.encode_literal(pg_st["mis_cnt"], pg_st["mis_sym"], pg_st["mis_rev_off"]))
    dec.set_text(dc["text"])
    dec.add_list_archive(hq["n"], st, hq["text_base"], off=hq["off"], rev_comp=hq["rc"])
    add_lists(dec, dc["lists"][1:])
    se = dec.writeAllReadsInSEMode()
    dec.close()
    plain = PgRCDecoder(L, device=0)
    plain.set_text(dc["text"])
    add_lists(plain, dc["lists"])                        # the original streams: context codes, rev-coded offsets
    assert np.array_equal(se, plain.writeAllReadsInSEMode())
    plain.close()
    truth = dc["truth"][pg_st["org_idx"].astype(np.int64)]
    assert np.array_equal(se[: truth.shape[0], :-1], truth)


# ---------------------------------------------------------------- refusals
def _swap_counts(st, changes):
    """the streams with some non-zero counts replaced: changes = [(old, new), ...], each applied to the first entry that has `old`"""
    nz = np.array(st["nonzero_cnt"], dtype=np.uint8)
    for old, new in changes:
        nz[np.flatnonzero(nz == old)[0]] = new
    return dict(st, nonzero_cnt=nz)


def test_add_list_archive_refusals_leave_the_context_usable():
    path = [p for p in la.fixtures() if la.case_name(p) == "mixed"][0]
    L, _, (cnt, sym, off, rev_off), st, (lcnt, lsym, loff) = la.load_case(path)
    n, text = cnt.size, text_for(cnt.size, L)
    want = rows_plain(L, text, lcnt, lsym, st["bases_order"], loff, False)
    props3 = np.array(st["props"], np.uint8)
    props3[2] = 3
    bad_sym = np.array(st["mis_sym"], np.uint8)
    bad_sym[100] = 4
    short = dict(st, props=np.array([5, 1, 2, 3, 4], np.uint8), dests=st["dests"][:6], n_mismatches=st["n_mismatches"])
    cases = [
        ("zero flags != n_nonzero", dict(st, n_nonzero=st["n_nonzero"] + 1, nonzero_cnt=np.concatenate([st["nonzero_cnt"], [1]]).astype(np.uint8)),
         "n_nonzero"),
        ("count above limit", _swap_counts(st, [(5, 7), (3, 1)]), "above the limit"),
        ("non-identity map", dict(st, props=props3), "identity"),
        ("limit above 254", dict(st, props=np.array([255] + list(range(1, 255)), np.uint8), n_dests=6), "254"),
        ("props_len", dict(st, props_len=5), "props_len"),
        ("dest_len != c * entries", _swap_counts(st, [(1, 2), (3, 2)]), "bytes for"),
        ("n_mismatches != sum of the counts", _swap_counts(st, [(1, 2)]), "sum to"),
        ("destinations != n_mismatches", short, "destinations hold"),
        ("n_entries", dict(st, n_entries=n - 1), "n_entries"),
        ("a code above 3", dict(st, mis_sym=bad_sym), "mismatch code"),
        ("a repeated symbol in bases_order", dict(st, bases_order=b"AACGT"), "bases_order"),
    ]
    dec = PgRCDecoder(L, device=0)
    dec.set_text(text)
    pos, rc = np.arange(n, dtype=np.uint64), (np.arange(n) % 3 == 0).astype(np.uint8)
    for what, bad, names in cases:
        with pytest.raises(PgrcMatchError) as e:
            dec.add_list_archive(n, bad, 0, pos=pos, rev_comp=rc)
        assert e.value.code == E_PARAM and names in str(e.value), (what, str(e.value))
        with pytest.raises(PgrcMatchError) as e2:          # no list was kept
            dec.set_order(pd.PGRC_DECODE_SE)
        assert e2.value.code == E_STATE, what
        assert np.array_equal(rows_archive(L, text, st, dec), want), what           # ... and the same context takes the good streams
        dec.set_text(text)
    # what pgrc_decode_add_list refuses: mis_* pointers beside the archive streams, a second list with mismatches, an offset
    # outside the read (the streams of L = 150 on a context of L = 20), a window past the text end
    a = pd.DecodeList()
    a.struct_size, a.n_entries = C.sizeof(pd.DecodeList), n
    a.pos, a.mis_cnt = pos.ctypes.data, cnt.ctypes.data
    s, keep = pd._list_archive_struct(st)
    assert lib.pgrc_decode_add_list_archive(dec._h, C.byref(a), C.byref(s)) == E_PARAM
    assert b"mis_*" in lib.pgrc_decode_last_error(dec._h)
    s.struct_size -= 8
    a.mis_cnt = None
    assert lib.pgrc_decode_add_list_archive(dec._h, C.byref(a), C.byref(s)) == E_PARAM
    assert lib.pgrc_decode_add_list_archive(dec._h, C.byref(a), None) == E_PARAM
    with pytest.raises(PgrcMatchError) as e:
        dec.add_list_archive(n, st, 0, pos=pos + np.uint64(L), rev_comp=rc)
    assert e.value.code == E_PARAM and "window" in str(e.value)
    dec.add_list_archive(n, st, 0, pos=pos, rev_comp=rc)
    with pytest.raises(PgrcMatchError) as e:
        dec.add_list_archive(n, st, 0, pos=pos)
    assert e.value.code == E_PARAM and "LQ and N" in str(e.value)
    assert np.array_equal(dec.writeAllReadsInSEMode(), want)
    dec.close()
    small = PgRCDecoder(20, device=0)
    small.set_text(text)
    with pytest.raises(PgrcMatchError) as e:
        small.add_list_archive(n, st, 0, pos=pos, rev_comp=rc)
    assert e.value.code == E_PARAM and "offset outside the read" in str(e.value)
    with pytest.raises(PgrcMatchError) as e:
        small.list_archive_timing()
    assert e.value.code == E_STATE
    small.close()


def _filled():
    s = ListArchiveStreams()
    C.memset(C.byref(s), 0x5A, C.sizeof(s))
    return s


def test_encode_refusals_clear_the_output_and_leave_the_context_usable():
    cnt, sym, rev_off = la.make_list(91, 5000, 150)
    good = la.encode_literal(cnt, sym, rev_off)
    low, high, c255 = sym.copy(), sym.copy(), cnt.copy()
    low[77] = 0x15
    high[4000] = 0x51
    first = int(np.flatnonzero(cnt == 1)[0])
    c255[first] = 255
    pad = np.zeros(254, np.uint8)
    cases = [("two-byte offsets", (cnt, sym, rev_off.astype(np.uint16)), None, False, "bytes"),
             ("n_mismatches above the counts' sum", (cnt, np.concatenate([sym, [1]]).astype(np.uint8), np.concatenate([rev_off, [0]]).astype(np.uint8)), None, False, "sum to"),
             ("n_mismatches below the counts' sum", (cnt, sym[:-1], rev_off[:-1]), None, True, "sum to"),
             ("a low nibble above 4", (cnt, low, rev_off), None, False, "nibble"),
             ("a high nibble above 4", (cnt, high, rev_off), None, True, "nibble"),
             ("a count of 255", (c255, np.concatenate([sym, pad + 1]), np.concatenate([rev_off, pad])), None, False, "255"),
             ("2^32 entries", (cnt, sym, rev_off), (1 << 32, sym.size), False, "2^32"),
             ("2^32 mismatches", (cnt, sym, rev_off), (cnt.size, 1 << 32), False, "2^32"),
             ("a NULL stream", (cnt, None, rev_off), (cnt.size, sym.size), False, "NULL")]
    dec = PgRCDecoder(150, device=0)
    for what, arrays, sizes, fast, names in cases:
        x, keep = pd._export_struct(arrays[0], arrays[1] if arrays[1] is not None else np.zeros(0, np.uint8), arrays[2])
        if sizes:
            x.n_entries, x.n_mismatches = sizes
        out = _filled()
        rc = lib.pgrc_list_archive_encode(dec._h, C.byref(x), int(fast), C.byref(out))
        msg = (lib.pgrc_decode_last_error(dec._h) or b"").decode()
        assert rc == E_PARAM and names in msg, (what, rc, msg)
        assert bytes(out) == bytes(C.sizeof(out)), what                # *out is cleared
        la.assert_streams(dec.list_archive_encode(cnt, sym, rev_off), good)        # ... and the same context codes a good list right away
    # at the fast level no count indexes the map: 255 is taken
    got = dec.list_archive_encode(c255, np.concatenate([sym, pad + 1]), np.concatenate([rev_off, pad]), True)
    assert got["props"].tobytes() == b"\1" and got["dests"][1].size == sym.size + 254 and got["nonzero_cnt"].max() == 255
    assert lib.pgrc_list_archive_encode(dec._h, None, 0, None) == E_PARAM
    out = _filled()
    assert lib.pgrc_list_archive_encode(dec._h, None, 0, C.byref(out)) == E_PARAM and bytes(out) == bytes(C.sizeof(out))
    dec.close()
