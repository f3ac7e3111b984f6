"""The order-preserving mode on the resident route (include/pgrc_readslist_ord.h: pgrc_rlist_export_original_order,
pgrc_rlist_archive_encode_ord, pgrc_rlist_positions; include/pgrc_decode.h: pgrc_decode_set_order_positions): the export equals
the committed "org" fixtures and the host route byte for byte, with the reads' indexes from the host and from read sets; its
edges against the oracle over export_util.original_order_entries; every refusal followed by a download of the earlier content;
the ORD archive block against the host archive form; the position array against tests/rlist_util narrowed as
tests/test_rlist_ord_reference.py pins it, and against what pair_positions implies; the decoder's entry against set_order; and the
chain divider -> read sets -> overlap -> assembly -> matcher -> export -> archive block -> positions -> decoder, single-file and
paired, whose rows are the source reads in source order."""
import ctypes as C

import numpy as np
import pytest

import decode_util as du
import export_util as xu
import listarchive_util as la
import rlist_util as rl
import rsets_util as ru
from pgrc_amd import (DividedPCLReadsSets, DividedReadsSets, MatchContext, OverlapFinder, PgAssembler, PgRCDecoder, PgrcMatchError,
                      ReadsList, _lib)
from test_gpu_decode import decoder, device_job
from test_gpu_listarchive import TILE
from test_gpu_rlist import matcher_with_results, refused, same_streams, simple_list
from test_gpu_rsets import chain_records
from test_rlist_ord_reference import SETTINGS, narrow_numpy
from util import gpu_match

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = 1, 6
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def sets_with_mappings(L, total, lq_idx, n_idx, seed=0):
    """read sets of `total` reads whose LQ and N mappings are the given (ascending) indexes, rows of random packed bytes"""
    rng = np.random.default_rng(seed)
    sym, rb = ru.set_shapes(L, True)
    counts = (total - lq_idx.size - n_idx.size, lq_idx.size, n_idx.size)
    rows = [rng.integers(0, 125 if sym[k] == 5 else 256, size=(c, rb[k]), dtype=np.uint8) for k, c in enumerate(counts)]
    st = {"A": int(total), "hq": rows[0], "lq": rows[1], "n": rows[2], "lq_map": np.concatenate([lq_idx, [total]]).astype(np.uint32),
          "n_map": np.concatenate([n_idx, [total]]).astype(np.uint32)}
    s = DividedReadsSets(L, True, False)
    s.append(ru.state_batch(st, L, True))
    s.finish()
    return s


# ------------------------------------------------------------------------------------------------ 1. the export and the reference
@pytest.mark.parametrize("name", xu.EXPORT_GOLDEN)
def test_export_equals_the_fixtures_and_the_host_route(name):
    case, pair, kmax, res, order, gold = xu.load_export_golden(name)
    g = gpu_match("c", case["pg"], case["reads"], 38, kmax, 0, n_nset=case["n_n"])
    ctx = g["ctx"]
    n, total = case["reads"].shape[0], case["total"]
    n_lq = n - case["n_n"]
    sets = sets_with_mappings(case["L"], total, case["read_org"][:n_lq], case["read_org"][n_lq:])
    assert np.array_equal(np.concatenate([sets.get_mapping("lq")[:-1], sets.get_mapping("n")[:-1]]), case["read_org"])
    lst = ReadsList(0)
    for byte_mode in (True, False):
        want = ctx.export_original_order(case["read_org"], total, pair, pair, byte_mode)
        assert want["last_pos"] == 0
        for from_sets in (False, True):
            lst.export_original_order(ctx, total, None if from_sets else case["read_org"], sets if from_sets else None, pair, pair, byte_mode)
            t = lst.timing()
            assert t["call"] == "export_original_order" and t["bytes_down"] == 0 and t["bytes_up"] == (0 if from_sets else 4 * n)
            got = lst.download()
            same_streams(got, want, (name, byte_mode, from_sets))
            i = lst.info()
            assert i["has_rev_comp"] and i["has_mismatches"] and i["off_width"] == (1 if byte_mode else 2) and i["last_pos"] == 0
            assert i["n_entries"] == got["org_idx"].size == total - int((g["mism"] == 255).sum()) and i["n_mismatches"] == got["mis_sym"].size
            if byte_mode:
                for k in xu.STREAMS:
                    assert np.ascontiguousarray(got[k]).tobytes() == gold["org"][k], (name, from_sets, k)
    for x in (lst, sets, ctx):
        x.close()


# ------------------------------------------------------------------------------------------------ 2. edges
def generated_case(seed, n, total, n_unmatched, G=30_000, L=100):
    """n reads that are Pg windows with up to two substitutions, half of them reverse-complemented, with the results a matcher
    would report for them written down (the last n_unmatched reads in a random order are unmatched), original indexes drawn from
    [0, total): the LQ part ascending, the N part (a fifth of the reads, none of which holds an N) ascending"""
    rng = np.random.default_rng(seed)
    pg = ACGT[rng.integers(0, 4, G)]
    pos = rng.integers(0, G - L + 1, n).astype(np.uint64)
    reads = pg[pos.astype(np.int64)[:, None] + np.arange(L)] if n else np.zeros((0, L), np.uint8)
    mism = np.zeros(n, np.uint8)
    for k in range(2):
        r = np.flatnonzero(rng.integers(0, 3, n) > k)
        c = 10 + 40 * k + rng.integers(0, 40, r.size)
        reads[r, c] = ACGT[(np.searchsorted(ACGT, reads[r, c]) + rng.integers(1, 4, r.size)) % 4]
        mism[r] += 1
    rc = (rng.random(n) < 0.5).astype(np.uint8)
    flip = rc.astype(bool)
    reads[flip] = du.revcomp_rows(reads[flip])
    un = rng.permutation(n)[:n_unmatched]
    pos[un], rc[un], mism[un] = rl.FILL, 0, 255
    idx = rng.permutation(total)[:n].astype(np.uint32)
    n_lq = n - n // 5
    read_org = np.concatenate([np.sort(idx[:n_lq]), np.sort(idx[n_lq:])]).astype(np.uint32)
    case = {"pg": pg, "reads": reads, "n_n": 0, "L": L, "read_org": read_org, "total": total, "n_lq": n_lq}
    return case, {"pos": pos, "rc": rc, "mism": mism}


def matcher_of(case, res):
    ctx = MatchContext(case["L"], 38, 33, 0, "c", device=0)
    ctx.set_pg_ascii(case["pg"])
    ctx.set_reads_ascii(case["reads"])
    ctx.init_results()
    if case["reads"].shape[0]:
        ctx.set_results(res["pos"], res["rc"], res["mism"])
    return ctx


def check_generated(case, res, pair_mode, pair_rule=False, byte_mode=True, lst=None, entries=None):
    er, eo = xu.original_order_entries(case["read_org"], res["mism"] != 255, case["total"], pair_mode, case["n_lq"])
    if entries is not None:
        assert er.size == entries
    want = xu.oracle_export_entries(case, res, er, eo, pair_file=pair_rule, byte_mode=byte_mode)
    ctx = matcher_of(case, res)
    own = lst is None
    lst = ReadsList(0) if own else lst
    lst.export_original_order(ctx, case["total"], case["read_org"], None, pair_mode, pair_rule, byte_mode)
    got = lst.download()
    assert got["org_idx"].size == er.size
    same_streams(got, dict(want, last_pos=0), (case["total"], pair_mode, pair_rule, byte_mode))
    assert np.array_equal(got["org_idx"], eo)
    ctx.close()
    if own:
        lst.close()
    return got


@pytest.mark.parametrize("entries", [4095, 4096, 4097])
def test_entry_counts_at_the_scan_edges(entries):
    total, n = 4300, 1500
    case, res = generated_case(entries, n, total, total - entries)
    got = check_generated(case, res, False, entries=entries)
    assert int(got["mis_cnt"].sum(dtype=np.int64)) > n // 3
    check_generated(case, res, True, True, False, entries=entries)


def test_edges_of_the_entry_list():
    # total 1: the one index is a matched read, an unmatched read (no entry at all), or nobody's (a filler)
    for n, un in ((1, 0), (1, 1), (0, 0)):
        case, res = generated_case(50 + n + un, n, 1, un)
        got = check_generated(case, res, False, entries=1 - un)
        assert n or (got["off"].size == 1 and got["off"][0] == 0 and not got["mis_cnt"].any())
    # a matcher with no reads: fillers alone, in class-major order with pair_file_mode
    case, res = generated_case(60, 0, 777, 0)
    for pair_mode in (False, True):
        got = check_generated(case, res, pair_mode, entries=777)
        assert not got["off"].any() and not got["rev_comp"].any() and got["mis_sym"].size == 0
    # every read matched and total == n: no filler; every read unmatched: total == n leaves nothing, a larger total fillers
    case, res = generated_case(61, 900, 900, 0)
    assert np.array_equal(np.sort(case["read_org"]), np.arange(900))
    check_generated(case, res, False, entries=900)
    check_generated(case, res, True, True, entries=900)
    case, res = generated_case(62, 300, 300, 300)
    check_generated(case, res, False, entries=0)
    case, res = generated_case(63, 300, 500, 300)
    check_generated(case, res, True, entries=200)
    # pair_file_mode with an odd total: one more even index than odd ones
    case, res = generated_case(64, 1000, 2501, 100)
    got = check_generated(case, res, True, True, entries=2401)
    assert got["org_idx"][0] == 0 and int((got["org_idx"] % 2 == 0).sum()) > int((got["org_idx"] % 2 == 1).sum())
    check_generated(case, res, True, False, False, entries=2401)
    # a list that held another content: replaced, not merged -- whatever it carried, mismatch streams included
    cnt, sym, rev_off = la.make_list(9, 3000, 100)
    lst = ReadsList(0)
    lst.set_host(np.full(3000, 7, np.uint16), np.arange(3000, dtype=np.uint32)[::-1], np.ones(3000, np.uint8), cnt, sym, rev_off.astype(np.uint16), last_pos=21000)
    check_generated(case, res, False, lst=lst, entries=2401)
    check_generated(case, res, True, True, lst=lst, entries=2401)          # ... and again over its own result
    lst.close()


# ------------------------------------------------------------------------------------------------ 3. refusals
def raw_export(lst, ctx, total, read_org, struct_size):
    a = _lib.RlistExportOrgArgs(struct_size)
    ro = np.ascontiguousarray(read_org, dtype=np.uint32)
    a.read_org_idx, a.reads_total_count, a.byte_per_read_length = ro.ctypes.data, total, 1
    return _lib.olib.pgrc_rlist_export_original_order(lst._h, ctx._h, C.byref(a)), (_lib.lib.pgrc_rlist_last_error(lst._h) or b"").decode()


def test_refusals_leave_the_list_as_it_was():
    case, res = generated_case(70, 1200, 2000, 150)
    ctx = matcher_of(case, res)
    ro, total, n = case["read_org"], case["total"], 1200
    cnt, sym, rev_off = la.make_list(3, 500, 100)
    lst = ReadsList(0)
    lst.set_host(np.arange(500, dtype=np.uint32).astype(np.uint8), np.arange(500, dtype=np.uint32), (np.arange(500) % 3 == 0).astype(np.uint8), cnt, sym, rev_off, last_pos=4711)
    kept = lst.download()
    refused(E_PARAM, lst.export_original_order, ctx, int(ro.max()), ro)                     # an index >= total
    same_streams(lst.download(), kept, "index >= total")
    dup = ro.copy()
    dup[1] = dup[0]
    refused(E_PARAM, lst.export_original_order, ctx, total, dup)                            # a shared index
    same_streams(lst.download(), kept, "shared index")
    sets = sets_with_mappings(100, total, ro[: case["n_lq"]], ro[case["n_lq"]:])
    refused(E_PARAM, lst.export_original_order, ctx, total, ro, sets)                       # both forms of the indexes
    same_streams(lst.download(), kept, "both forms")
    refused(E_PARAM, lst.export_original_order, ctx, total)                                 # ... and neither
    other = sets_with_mappings(100, total, ro[: case["n_lq"] - 1], ro[case["n_lq"]:])
    refused(E_PARAM, lst.export_original_order, ctx, total, None, other)                    # sets of another count
    same_streams(lst.download(), kept, "sets of another count")
    refused(E_PARAM, lst.export_original_order, ctx, 0xFFFFFFFE, ro)                        # too many indexes
    many = MatchContext(100, 38, 33, 0, "c", devices=[0, 0])
    refused(E_PARAM, lst.export_original_order, many, total, ro)                            # a matcher over several shards
    many.close()
    fresh = MatchContext(100, 38, 33, 0, "c", device=0)
    refused(E_STATE, lst.export_original_order, fresh, total, ro)                           # no run
    fresh.set_pg_ascii(case["pg"])
    fresh.set_reads_ascii(case["reads"])
    refused(E_STATE, lst.export_original_order, fresh, total, ro)                           # reads, but no results
    fresh.close()
    same_streams(lst.download(), kept, "matchers without results")
    code, msg = raw_export(lst, ctx, total, ro, C.sizeof(_lib.RlistExportOrgArgs) - 8)      # a wrong struct_size, named
    assert code == E_PARAM and "pgrc_rlist_export_org_args" in msg
    o = _lib.RlistPositionsOut(C.sizeof(_lib.RlistPositionsOut) + 8)
    p = _lib.RlistPairPosArgs(C.sizeof(_lib.RlistPairPosArgs), 8, 500)
    p.hq = lst._h
    assert _lib.olib.pgrc_rlist_positions(C.byref(p), C.byref(o)) == E_PARAM and b"pgrc_rlist_positions_out" in _lib.lib.pgrc_rlist_last_error(lst._h)
    same_streams(lst.download(), kept, "after the refusals")
    # ... and the object is usable: a good call, from the host and from the sets
    want = ctx.export_original_order(ro, total)
    lst.export_original_order(ctx, total, ro)
    same_streams(lst.download(), want, "a good call after them")
    lst.export_original_order(ctx, total, sets=sets)
    same_streams(lst.download(), want, "from the sets")
    for x in (lst, sets, other, ctx):
        x.close()


def test_a_matcher_on_another_device_is_refused():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    case, res = generated_case(71, 200, 300, 10)
    lst = simple_list(np.arange(5, dtype=np.uint32))
    kept = lst.download()
    far = MatchContext(100, 38, 33, 0, "c", device=1)
    far.set_pg_ascii(case["pg"])
    far.set_reads_ascii(case["reads"])
    far.init_results()
    refused(E_PARAM, lst.export_original_order, far, 300, case["read_org"])
    both = MatchContext(100, 38, 33, 0, "c", devices=[0, 1])
    refused(E_PARAM, lst.export_original_order, both, 300, case["read_org"])
    same_streams(lst.download(), kept)
    for x in (far, both, lst):
        x.close()


# ------------------------------------------------------------------------------------------------ 4. the ORD archive form
def ord_archive(dec, cnt, sym, rev_off, fast):
    n = cnt.size
    rng = np.random.default_rng(n)
    rc = (rng.random(n) < 0.5).astype(np.uint8)
    lst = ReadsList(0)
    lst.set_host(rng.integers(0, 250, size=n).astype(np.uint8), rng.permutation(n).astype(np.uint32), rc, cnt, sym, rev_off)
    down = lst.download()
    got = lst.archive_encode_ord(fast)
    assert got["off"] is None and got["org_idx"] is None and got["block_start"] == "rev_comp" and got["n_entries"] == n and got["off_width"] == 1
    assert np.array_equal(got["rev_comp"], down["rev_comp"]) and np.array_equal(got["rev_comp"], rc)
    want = dec.list_archive_encode(down["mis_cnt"], down["mis_sym"], down["mis_rev_off"], fast)
    la.assert_streams(got["archive"], want)
    # one block that holds revComp and the archive part: the streams, an alignment gap and at most 16 bytes behind each
    assert got["one_block"] and got["archive"]["one_block"]
    streams = n + n + int(want["n_nonzero"]) + 2 * sym.size
    assert streams <= got["block_bytes"] <= streams + 8 * 32
    t = lst.timing()
    assert t["call"] == "archive_encode" and t["bytes_up"] == 0 and t["bytes_down"] == got["block_bytes"]
    same_streams(lst.download(), down, "the list after its archive form")
    lst.close()
    return got


@pytest.mark.parametrize("path", la.fixtures(), ids=la.case_name)
def test_ord_archive_form_of_the_fixtures(path):
    L, fast, (cnt, sym, off, rev_off), st, _ = la.load_case(path)
    dec = PgRCDecoder(L, device=0)
    la.assert_streams(ord_archive(dec, cnt, sym, rev_off, fast)["archive"], st)
    if not fast:
        ord_archive(dec, cnt, sym, rev_off, True)          # (the fast level has one destination and takes every list)
    dec.close()


@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1])
def test_ord_archive_form_around_the_tile(n):
    L = 40
    cnt, sym, rev_off = la.make_list(8100 + n % 977, n, L)
    dec = PgRCDecoder(L, device=0)
    for fast in (False, True):
        la.assert_streams(ord_archive(dec, cnt, sym, rev_off, fast)["archive"], la.encode_literal(cnt, sym, rev_off, fast))
    dec.close()


def test_ord_archive_form_refusals():
    cnt, sym, rev_off = la.make_list(6, 300, 40)
    off, org, rc = np.zeros(300, np.uint8), np.arange(300, dtype=np.uint32), np.ones(300, np.uint8)
    lst = ReadsList(0)
    for args, code in (((off, org), E_STATE), ((off, org, rc), E_STATE),                       # no mismatch streams
                       ((off, org, None, cnt, sym, rev_off), E_STATE),                          # no RC flags
                       ((off.astype(np.uint16), org, rc, cnt, sym, rev_off.astype(np.uint16)), E_PARAM)):      # offsets of two bytes
        lst.set_host(*args)
        kept = lst.download()
        refused(code, lst.archive_encode_ord)
        same_streams(lst.download(), kept)
    bad = sym.copy()
    bad[bad.size // 2] = 0x05                                                                   # what pgrc_list_archive_encode refuses
    lst.set_host(off, org, rc, cnt, bad, rev_off)
    refused(E_PARAM, lst.archive_encode_ord)
    lst.set_host(off, org, rc, cnt, sym, rev_off)
    assert lst.archive_encode_ord()["archive"]["n_mismatches"] == sym.size
    lst.close()


# ------------------------------------------------------------------------------------------------ 5. positions
def setting_lists(s):
    lists = {k: (ReadsList(0) if s[k] is not None else None) for k in ("hq", "lq", "n")}
    for k, l in lists.items():
        if l is not None:
            l.set_host(s[k][0], s[k][1])
    ctx, pos = matcher_with_results(s["read_org"].size, s["match_pos"])
    ro = np.zeros(pos.size, np.uint32)
    ro[: s["read_org"].size] = s["read_org"]
    return lists, ctx, ro


def close_all(lists, ctx):
    ctx.close()
    for l in lists.values():
        if l is not None:
            l.close()


@pytest.mark.parametrize("seed,T", SETTINGS)
def test_positions_of_seeded_settings(seed, T):
    s = rl.make_setting(seed, T=T)
    want = rl.positions_of(s, rl.positions_literal)
    lists, ctx, ro = setting_lists(s)
    args = (s["T"], lists["lq"], lists["n"], s["hq_len"], s["lq_len"], ctx, ro)
    hq = lists["hq"]
    got = hq.positions(args[0], 8, *args[1:])
    assert got.dtype == np.uint64 and np.array_equal(got, narrow_numpy(want, 8))
    t = hq.timing()
    assert t["call"] == "positions" and t["bytes_up"] == 4 * ro.size and t["bytes_down"] == 8 * s["T"]
    if int(want.max(initial=0)) < 2**32:
        got = hq.positions(args[0], 4, *args[1:])
        assert got.dtype == np.uint32 and np.array_equal(got, narrow_numpy(want, 4))
        assert hq.timing()["bytes_down"] == 4 * s["T"]
    else:
        refused(E_PARAM, hq.positions, args[0], 4, *args[1:])
        assert np.array_equal(hq.positions(args[0], 8, *args[1:]), want)            # the handle works after the refusal
    # at an even T the array is what pair_positions implies: its streams decoded are the array de-interleaved
    if s["T"] % 2 == 0:
        dec = PgRCDecoder(100, device=0)
        for W in (8, 4) if int(want.max(initial=0)) < 2**32 else (8,):
            file_major = dec.decompressReadsPgPositions(hq.pair_positions(args[0], W, *args[1:]))
            arr = hq.positions(args[0], W, *args[1:]).astype(np.uint64)
            assert np.array_equal(file_major[: s["T"] // 2], arr[0::2]) and np.array_equal(file_major[s["T"] // 2:], arr[1::2])
        dec.close()
    else:
        refused(E_PARAM, hq.pair_positions, args[0], 8, *args[1:])                  # (the paired call wants an even total)
    close_all(lists, ctx)


def test_positions_of_no_reads():
    """T = 0: three empty lists and no matcher give an empty array in a block of no bytes; one entry too many is refused"""
    empty = np.zeros(0, np.uint32)
    lists = [simple_list(empty) for _ in range(3)]
    for W, dt in ((4, np.uint32), (8, np.uint64)):
        got = lists[0].positions(0, W, lists[1], lists[2], 100, 100)
        assert got.dtype == dt and got.size == 0
        t = lists[0].timing()
        assert t["call"] == "positions" and t["bytes_down"] == 0 and t["bytes_up"] == 0
    assert lists[0].positions(0, 8).size == 0                                        # the HQ list alone
    refused(E_PARAM, lists[0].positions, 0, 8, simple_list(np.zeros(1, np.uint32)))
    assert lists[0].positions(0, 4).size == 0
    for l in lists:
        l.close()


def test_positions_refusals():
    """an odd T dealt to three lists and a matcher; the constructions of test_gpu_rlist's pair-position refusals"""
    rng = np.random.default_rng(17)
    sizes, n_matched = [1501, 700, 300], 500
    T = n_matched + sum(sizes)
    assert T % 2 == 1
    perm = rng.permutation(T).astype(np.uint32)
    ctx, mpos = matcher_with_results(n_matched + 3, rng.integers(0, 3000, size=n_matched).astype(np.uint64))
    read_org = np.zeros(mpos.size, np.uint32)
    read_org[:n_matched] = perm[:n_matched]
    at, lists, host = n_matched, [], []
    for n in sizes:
        off, org = rng.integers(0, 120, size=n).astype(np.uint8), perm[at: at + n]
        at += n
        lists.append(simple_list(org, off))
        host.append((off, org))
    hq_len, lq_len = int(host[0][0].sum()) + 100, int(host[1][0].sum()) + 100
    want = rl.positions_literal(T, host[0], host[1], host[2], hq_len, lq_len, read_org, mpos)
    good = (lists[1], lists[2], hq_len, lq_len, ctx, read_org)
    hq = lists[0]
    assert np.array_equal(hq.positions(T, 4, *good), narrow_numpy(want, 4))
    org2 = host[2][1].copy()
    org2[0] = host[1][1][0]
    refused(E_PARAM, hq.positions, T, 8, lists[1], simple_list(org2, host[2][0]), hq_len, lq_len, ctx, read_org)       # an index written twice
    refused(E_PARAM, hq.positions, T, 8, lists[1], None, hq_len, lq_len, ctx, read_org)                                # the N list's are never written
    refused(E_PARAM, hq.positions, T + 1, 8, *good)
    refused(E_PARAM, hq.positions, T - 1, 8, *good)
    org3 = host[2][1].copy()
    org3[5] = T
    refused(E_PARAM, hq.positions, T, 8, lists[1], simple_list(org3, host[2][0]), hq_len, lq_len, ctx, read_org)       # an index of T
    refused(E_PARAM, hq.positions, T, 4, lists[1], lists[2], 2**32, lq_len, ctx, read_org)                             # 2^32 in four bytes
    refused(E_PARAM, hq.positions, T, 5, *good)
    refused(E_PARAM, hq.positions, T, 8, lists[1], lists[2], hq_len, lq_len, ctx, read_org, DividedReadsSets(100, True, False))
    fresh = MatchContext(100, 38, 3, 0, "c", device=0)
    refused(E_STATE, hq.positions, T, 8, lists[1], lists[2], hq_len, lq_len, fresh, read_org)
    fresh.close()
    same_streams(hq.download(), {"off": host[0][0], "org_idx": host[0][1], "rev_comp": np.zeros(sizes[0], np.uint8), "mis_cnt": np.zeros(sizes[0], np.uint8),
                                 "mis_sym": np.zeros(0, np.uint8), "mis_rev_off": np.zeros(0, np.uint8), "last_pos": 0})
    assert np.array_equal(hq.positions(T, 8, *good), want)
    ctx.close()
    for l in lists:
        l.close()


# ------------------------------------------------------------------------------------------------ 6. the decoder's entry
@pytest.fixture(scope="module")
def ord_job():
    case, res, pg_st, org_st = device_job(140, 100, False, G=60_000, n=2500, n_with_n=60)
    return du.decode_case(case, res, pg_st, org_st, pair=False)


@pytest.mark.parametrize("rule", [False, True])
def test_set_order_positions_equals_set_order(ord_job, rule):
    dc = ord_job
    pos = dc["org2pos"]
    assert pos.dtype == np.uint64 and int(pos.max()) < 2**32 and pos.size == dc["T"]
    dec = decoder(dc, dc["ord_lists"])
    dec.set_order(2, pos.size, org_idx_to_pos=pos, rev_compl_pair_file=rule)
    want = dec.rows(0).copy()
    if not rule:
        assert np.array_equal(want, du.truth_rows_ord(dc, dc["text"], 0, False))
    for dt in (np.uint32, np.uint64):
        dec.set_order(0)                                        # (another order in between: nothing is left over)
        dec.set_order_positions(pos.astype(dt), rule)
        assert dec.row_count(0) == pos.size and np.array_equal(dec.rows(0), want), dt
    dec.close()


def test_set_order_positions_refusals(ord_job):
    dc = ord_job
    pos = dc["org2pos"].astype(np.uint32)
    dec = decoder(dc, dc["ord_lists"])
    bad = pos.copy()
    bad[1] = dc["text"].size - dc["L"] + 1                      # a window past the text end
    for arr in (bad, bad.astype(np.uint64), pos.astype(np.uint16), pos.astype(np.uint8)):
        dec.set_order_positions(pos)
        refused(E_PARAM, dec.set_order_positions, arr)
        refused(E_STATE, dec.rows, 0)                           # the context has no order
    assert _lib.lib.pgrc_decode_set_order_positions(dec._h, None, 4, 5, 0) == E_PARAM
    refused(E_STATE, dec.rows, 0)
    dec.set_order_positions(pos)
    assert np.array_equal(dec.rows(0), du.truth_rows_ord(dc, dc["text"], 0, False))
    empty = PgRCDecoder(dc["L"], device=0)
    refused(E_STATE, empty.set_order_positions, pos)            # no list
    for x in (dec, empty):
        x.close()


# ------------------------------------------------------------------------------------------------ 7. the chain
@pytest.mark.parametrize("paired", [False, True])
def test_chain_from_the_assembly_to_the_decoder(paired):
    """4000 reads of 100 bp: the encoder's second half in the order-preserving mode without a list array crossing the link
    upwards, then a decoder fed with nothing but the blocks that came down.  The decoder's rows are the source reads in source
    order; in the paired mode file p holds the reads 2i + p, and the rows of file 2 that come from the LQ and N pseudogenomes
    are reverse-complemented by the decoder's writer (decode_util.write_ord), as the reference's is."""
    L = 100
    genome, reads, quals = chain_records(n=4000, L=L)
    T = reads.shape[0]
    div = DividedPCLReadsSets(L, 0.05, True, True, False)
    div.divide(reads, quals)
    sets = DividedReadsSets(L, True, False)
    sets.append_divider(div)
    sets.finish()
    ovl, asm = OverlapFinder(), PgAssembler(device=0)
    sets.overlap("hq", ovl, 0.6)
    sets.move_by_overlap(ovl)
    sets.overlap("hq", ovl, 0.6)
    hq = ReadsList(0)
    hq.from_overlap(ovl, asm, sets, "hq")
    ctx = MatchContext(L, 38, 3, 0, "c", device=0)
    ctx.set_pg_packed_device(asm.packed_device(), asm.pg_len)
    sets.to_matcher(ctx)
    ctx.init_results()
    ctx.run(True)
    mpos = ctx.get_results()[0]
    n_matched = int((mpos != rl.FILL).sum())
    assert 0 < n_matched < mpos.size
    read_org = np.concatenate([sets.get_mapping("lq")[:-1], sets.get_mapping("n")[:-1]])
    # the export into a second list (the HQ list stays for the positions), the indexes read from the read sets
    exp = ReadsList(0)
    exp.export_original_order(ctx, T, None, sets, paired, False, True)
    t = exp.timing()
    assert t["call"] == "export_original_order" and t["bytes_up"] == 0 and t["bytes_down"] == 0
    same_streams(exp.download(), ctx.export_original_order(read_org, T, paired, False, True), "export")
    assert exp.info()["n_entries"] == T - (mpos.size - n_matched) and exp.info()["n_mismatches"] > 0
    arch = exp.archive_encode_ord()
    t = exp.timing()
    assert t["bytes_up"] == 0 and t["bytes_down"] == arch["block_bytes"] and arch["one_block"] and arch["off"] is None and arch["org_idx"] is None
    # the LQ and the N pseudogenome of what the matcher left, their lists mapped from the read sets
    sets.remove_matched(ctx)
    rest, texts = [], [asm.text()]
    for which in ("lq", "n"):
        sets.overlap(which, ovl, 0.6)
        a = PgAssembler(device=0)
        lst = ReadsList(0)
        lst.from_overlap(ovl, a, sets, which)
        assert lst.timing()["bytes_up"] == 0 and lst.info()["n_entries"] > 0
        rest.append(lst)
        texts.append(a.text())
        a.close()
    hq_len, lq_len = texts[0].size, texts[1].size
    text = np.concatenate(texts)
    W = 4
    dec = PgRCDecoder(L, device=0)
    dec.set_text(text)
    dec.add_list_archive(arch["n_entries"], arch["archive"], 0, rev_comp=arch["rev_comp"])
    dec.add_list(rest[0].info()["n_entries"], hq_len)
    dec.add_list(rest[1].info()["n_entries"], hq_len + lq_len)
    if not paired:
        pos = hq.positions(T, W, rest[0], rest[1], hq_len, lq_len, ctx, read_org)
        t = hq.timing()
        assert pos.dtype == np.uint32 and t["bytes_down"] == 4 * T and t["bytes_up"] == 4 * read_org.size
        dec.set_order_positions(pos)
        assert np.array_equal(dec.rows(0), du.with_newlines(reads))
    else:
        streams = hq.pair_positions(T, W, rest[0], rest[1], hq_len, lq_len, ctx, read_org)
        dec.set_order_pair_streams(streams, False)
        file_major = dec.decompressReadsPgPositions(streams)
        for p in range(2):
            want = reads[p::2].copy()
            from_rest = file_major[p * (T // 2): (p + 1) * (T // 2)] >= hq_len
            assert 0 < int(from_rest.sum()) < T // 2
            if p == 1:
                want[from_rest] = du.revcomp_rows(want[from_rest])
            assert np.array_equal(dec.rows(p), du.with_newlines(want)), p
    for x in [hq, exp, ctx, dec, ovl, asm, sets, div] + rest:
        x.close()
