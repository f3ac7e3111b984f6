"""A pseudogenome's reads list kept on the device (include/pgrc_readslist.h, pgrc_amd.ReadsList; pgrc_amd/csrc/rlist.hip): the
resident route equals the host route made from the existing entry points byte for byte, and the committed fixtures where there
are any -- the round trip, the export (the tie rule, offsets of two bytes, the order made on the device), the archive form (the
split's tile +- 1, no mismatches, one entry), the assembly with applyIndexesMapping read from the read sets, the pair order in
all four forms, the pair positions against tests/rlist_util -- every refusal followed by a download of the earlier content, and
the chain divider -> read sets -> overlap -> assembly -> matcher -> export -> archive form -> pair order without a list array
going up and with the archive block alone coming down."""
import os

import numpy as np
import pytest

import export_util as xu
import listarchive_util as la
import pairorder_util as po
import pairpos_util as pp
import rlist_util as rl
import rsets_util as ru
from pgrc_amd import (DividedPCLReadsSets, DividedReadsSets, MatchContext, OverlapFinder, PgAssembler, PgRCDecoder, PgrcMatchError,
                      ReadsList)
from test_gpu_listarchive import TILE
from test_gpu_pairorder import assert_streams as assert_pairorder
from test_gpu_pairpos import assert_streams as assert_pairpos
from test_gpu_rsets import chain_records
from test_pairorder_oracle import FIXTURES as PAIRORDER_FIXTURES, case_name as pairorder_name, load_case as load_pairorder
from test_pairpos_oracle import FIXTURES as PAIRPOS_FIXTURES, load_case as load_pairpos
from test_pgasm_oracle import FIXTURES as PGASM_FIXTURES, case_name as pgasm_name, load_case as load_pgasm
from util import gpu_match

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = 1, 6


def same_streams(got, want, what=""):
    for k in xu.STREAMS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.size == w.size and g.tobytes() == w.tobytes(), (what, k)
    assert int(got["last_pos"]) == int(want["last_pos"]), what


def refused(code, fn, *a, **kw):
    with pytest.raises(PgrcMatchError) as e:
        fn(*a, **kw)
    assert e.value.code == code, str(e.value)


def simple_list(org, off=None, device=0):
    org = np.ascontiguousarray(org, dtype=np.uint32)
    lst = ReadsList(device)
    lst.set_host(np.zeros(org.size, np.uint8) if off is None else off, org)
    return lst


# ------------------------------------------------------------------------------------------------ set_host -> download
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 255, 4097])
def test_set_host_download_round_trip(n):
    rng = np.random.default_rng(n)
    lst = ReadsList(0)
    assert lst.info() == {"off_width": 1, "n_entries": 0, "n_mismatches": 0, "last_pos": 0, "has_rev_comp": False, "has_mismatches": False}
    refused(E_STATE, lst.timing)
    for ot in (np.uint8, np.uint16):
        for with_rc in (False, True):
            for with_mis in (False, True):
                off = rng.integers(0, 250 if ot == np.uint8 else 60000, size=n).astype(ot)
                org = rng.permutation(n).astype(np.uint32)
                rc = (rng.random(n) < 0.5).astype(np.uint8)
                cnt = rng.integers(0, 4, size=n).astype(np.uint8)
                m = int(cnt.sum())
                sym = ((rng.integers(0, 5, size=m) << 4) + rng.integers(0, 5, size=m)).astype(np.uint8)
                roff = rng.integers(0, 200, size=m).astype(ot)
                lst.set_host(off, org, rc if with_rc else None, *((cnt, sym, roff) if with_mis else (None, None, None)), last_pos=12345 + n)
                want = {"off": off, "org_idx": org, "rev_comp": rc if with_rc else np.zeros(n, np.uint8), "mis_cnt": cnt if with_mis else np.zeros(n, np.uint8),
                        "mis_sym": sym if with_mis else np.zeros(0, np.uint8), "mis_rev_off": roff if with_mis else np.zeros(0, ot), "last_pos": 12345 + n}
                same_streams(lst.download(), want, (n, ot, with_rc, with_mis))
                i = lst.info()
                assert (i["n_entries"], i["n_mismatches"], i["off_width"], i["has_rev_comp"], i["has_mismatches"]) == (n, m if with_mis else 0, np.dtype(ot).itemsize, with_rc, with_mis)
                t = lst.timing()
                assert t["call"] == "download" and t["bytes_up"] == 0 and t["bytes_down"] == sum(np.asarray(want[k]).nbytes for k in xu.STREAMS if (k != "rev_comp" or with_rc) and (with_mis or not k.startswith("mis_")))
    # the refusals leave the list as it was
    if n:
        kept = lst.download()
        refused(E_PARAM, lst.set_host, off, org, None, cnt, None, None)                              # one of the three streams
        if m:
            refused(E_PARAM, lst.set_host, off, org, None, cnt, sym, None)                           # two of them
            refused(E_PARAM, lst.set_host, off, org, None, cnt, sym[:-1], roff[:-1])                 # n_mismatches is not the counts' sum
            refused(E_PARAM, lst.set_host, off, org, None, None, None, None, 0, m)                   # mismatches without streams
        same_streams(lst.download(), kept, "after the refusals")
    lst.close()


# ------------------------------------------------------------------------------------------------ the export
def resident_export(case, ctx, order, pair, byte_mode, with_rc=True, with_org=True):
    lst = ReadsList(0)
    lst.set_host(case["list_off"], case["list_org"], case["list_rc"] if with_rc else None)
    lst.export_pg_order(ctx, order, case["read_org"] if with_org else None, None, pair, byte_mode)
    t = lst.timing()
    assert t["call"] == "export_pg_order" and t["bytes_down"] == 0
    assert t["bytes_up"] == (0 if order is None else 4 * np.asarray(order).size) + (4 * case["read_org"].size if with_org else 0)
    got = lst.download()
    i = lst.info()
    assert i["has_rev_comp"] and i["has_mismatches"] and i["off_width"] == (1 if byte_mode else 2) and i["n_entries"] == got["org_idx"].size
    return lst, got


@pytest.mark.parametrize("name", xu.EXPORT_GOLDEN)
def test_export_equals_the_fixtures_and_the_host_route(name):
    case, pair, kmax, res, order, gold = xu.load_export_golden(name)
    g = gpu_match("c", case["pg"], case["reads"], 38, kmax, 0, n_nset=case["n_n"])
    ctx = g["ctx"]
    lst, got = resident_export(case, ctx, order, pair, True)
    want = ctx.export_pg_order(order, case["list_off"], case["list_org"], case["list_rc"], case["read_org"], pair, True)
    same_streams(got, want, name)
    for k in xu.STREAMS:
        assert np.ascontiguousarray(got[k]).tobytes() == gold["pg"][k], (name, k)
    # a second export into a list that carries mismatches is refused and changes nothing
    refused(E_STATE, lst.export_pg_order, ctx, order, case["read_org"], None, pair, True)
    same_streams(lst.download(), want, "after the refusal")
    lst.close()
    # offsets of two bytes (L = 250 has them in the reference's runs), no RC flags on the old list, identity indexes
    for byte_mode, with_rc, with_org in ((False, True, True), (True, False, False)) if name in ("export_L250", "export_se") else ():
        lst, got = resident_export(case, ctx, order, pair, byte_mode, with_rc, with_org)
        want = ctx.export_pg_order(order, case["list_off"], case["list_org"], case["list_rc"] if with_rc else None, case["read_org"] if with_org else None, pair, byte_mode)
        assert got["off"].dtype == (np.uint8 if byte_mode else np.uint16)
        same_streams(got, want, (name, byte_mode, with_rc, with_org))
        lst.close()
    # the order made on the device
    if name in ("export_se", "export_pe_pairfile"):
        lst, got = resident_export(case, ctx, None, pair, True)
        same_streams(got, ctx.export_pg_order(None, case["list_off"], case["list_org"], case["list_rc"], case["read_org"], pair, True), (name, "order_on_device"))
        lst.close()


def test_export_tie_rule_and_refusals():
    case, pair, kmax, res, order, _ = xu.load_export_golden("export_se")
    g = gpu_match("c", case["pg"], case["reads"], 38, kmax, 0, n_nset=case["n_n"])
    ctx = g["ctx"]
    # an old entry at the position of a matched read: the new entry goes first (SeparatedPseudoGenomePersistence.cpp:1004-1019)
    p = int(res["pos"][order[order.size // 2]])
    off = case["list_off"].copy()
    lp = np.cumsum(off.astype(np.int64))
    k = int(np.searchsorted(lp, p, side="right"))
    assert 0 < k < off.size - 1 and lp[k] - p < off[k]
    d = int(lp[k] - p)
    off[k] -= d
    off[k + 1] += d
    assert np.cumsum(off.astype(np.int64))[k] == p
    tie = dict(case, list_off=off)
    lst, got = resident_export(tie, ctx, order, pair, True)
    want = ctx.export_pg_order(order, off, case["list_org"], case["list_rc"], case["read_org"], pair, True)
    same_streams(got, want, "tie")
    same_streams(got, xu.oracle_export_pg_order(tie, res, order), "tie against the oracle")
    at = np.flatnonzero(np.cumsum(got["off"].astype(np.int64)) == p)
    assert at.size >= 2 and got["org_idx"][at[-1]] == case["list_org"][k]          # the old entry is the last one at p
    lst.close()
    # refusals: the list stays what set_host made it
    lst = ReadsList(0)
    lst.set_host(case["list_off"], case["list_org"], case["list_rc"])
    kept = lst.download()
    unmatched = np.flatnonzero(res["mism"] == 255)[:1].astype(np.uint32)
    refused(E_PARAM, lst.export_pg_order, ctx, unmatched, case["read_org"])                          # order[] names a read without a match
    refused(E_PARAM, lst.export_pg_order, ctx, np.array([case["reads"].shape[0]], np.uint32))       # a read index out of range
    many = MatchContext(case["L"], 38, kmax, 0, "c", devices=[0, 0])
    refused(E_PARAM, lst.export_pg_order, many, order)                                               # a matcher on several devices
    many.close()
    fresh = MatchContext(case["L"], 38, kmax, 0, "c", device=0)
    refused(E_STATE, lst.export_pg_order, fresh, order)                                              # no run
    fresh.close()
    sets = DividedReadsSets(case["L"], True, False)
    sets.append(ru.state_batch(ru.state_with_counts(np.random.default_rng(1), case["L"], True, (5, 7, 3)), case["L"], True))
    sets.finish()
    refused(E_PARAM, lst.export_pg_order, ctx, order, case["read_org"], sets)                        # the indexes given twice
    refused(E_PARAM, lst.export_pg_order, ctx, order, None, sets)                                    # sets of another count
    sets.close()
    same_streams(lst.download(), kept, "after the refusals")
    lst.export_pg_order(ctx, order, case["read_org"])
    same_streams(lst.download(), ctx.export_pg_order(order, case["list_off"], case["list_org"], case["list_rc"], case["read_org"]), "a good call after them")
    lst.close()


# ------------------------------------------------------------------------------------------------ the archive form
def archive_both_routes(dec, cnt, sym, rev_off, fast, with_rc=True, want_org=True, off_dtype=np.uint8):
    n = cnt.size
    rng = np.random.default_rng(n)
    off = rng.integers(0, 250, size=n).astype(off_dtype)
    org, rc = rng.permutation(n).astype(np.uint32), (rng.random(n) < 0.5).astype(np.uint8)
    lst = ReadsList(0)
    lst.set_host(off, org, rc if with_rc else None, cnt, sym, rev_off)
    got = lst.archive_encode(fast, want_org)
    assert got["one_block"] and got["n_entries"] == n
    assert got["off"].dtype == off_dtype and np.array_equal(got["off"], off)
    assert (got["rev_comp"] is None) == (not with_rc) and (not with_rc or np.array_equal(got["rev_comp"], rc))
    assert (got["org_idx"] is None) == (not want_org) and (not want_org or np.array_equal(got["org_idx"], org))
    t = lst.timing()
    assert t["call"] == "archive_encode" and t["bytes_up"] == 0 and t["bytes_down"] == got["block_bytes"]
    if cnt is not None:
        want = dec.list_archive_encode(cnt, sym, rev_off, fast)
        la.assert_streams(got["archive"], want)
        assert got["archive"]["one_block"]
        # the block holds the streams and padding only: at most 16 bytes and an alignment gap per stream
        streams = n * off.itemsize + (n if with_rc else 0) + (4 * n if want_org else 0) + n + int(want["n_nonzero"]) + 2 * sym.size
        assert streams <= got["block_bytes"] <= streams + 8 * 32
    lst.close()
    return got


@pytest.mark.parametrize("path", la.fixtures(), ids=la.case_name)
def test_archive_form_equals_the_fixtures_and_the_host_route(path):
    L, fast, (cnt, sym, off, rev_off), st, _ = la.load_case(path)
    dec = PgRCDecoder(L, device=0)
    got = archive_both_routes(dec, cnt, sym, rev_off, fast)
    la.assert_streams(got["archive"], st)
    archive_both_routes(dec, cnt, sym, rev_off, fast, with_rc=False, want_org=False)
    dec.close()


@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1])
def test_archive_form_around_the_tile(n):
    L = 40
    cnt, sym, rev_off = la.make_list(7100 + n % 977, n, L)
    dec = PgRCDecoder(L, device=0)
    for fast in (False, True):
        got = archive_both_routes(dec, cnt, sym, rev_off, fast, with_rc=bool(n % 2), want_org=not fast)
        la.assert_streams(got["archive"], la.encode_literal(cnt, sym, rev_off, fast))
    dec.close()


def test_archive_form_of_lists_without_mismatches_and_refusals():
    rng = np.random.default_rng(3)
    for n, ot in ((0, np.uint8), (1, np.uint8), (1000, np.uint8), (1000, np.uint16)):
        off, org = rng.integers(0, 250, size=n).astype(ot), rng.permutation(n).astype(np.uint32)
        lst = ReadsList(0)
        lst.set_host(off, org)
        got = lst.archive_encode(False, True)
        assert got["archive"] is None and got["rev_comp"] is None and np.array_equal(got["off"], off) and np.array_equal(got["org_idx"], org)
        assert got["off"].dtype == ot and got["block_bytes"] == lst.timing()["bytes_down"] and (n == 0 or got["block_bytes"] >= n * (4 + np.dtype(ot).itemsize))
        got = lst.archive_encode(False, False)
        assert got["org_idx"] is None and got["block_bytes"] == n * np.dtype(ot).itemsize
        lst.close()
    # what pgrc_list_archive_encode refuses: offsets of two bytes, a count of 255, a nibble above 4
    cnt, sym, rev_off = la.make_list(5, 300, 40)
    lst = ReadsList(0)
    lst.set_host(np.zeros(300, np.uint16), np.arange(300, dtype=np.uint32), None, cnt, sym, rev_off.astype(np.uint16))
    kept = lst.download()
    refused(E_PARAM, lst.archive_encode)
    same_streams(lst.download(), kept)
    bad = sym.copy()
    bad[bad.size // 2] = 0x05
    lst.set_host(np.zeros(300, np.uint8), np.arange(300, dtype=np.uint32), None, cnt, bad, rev_off)
    kept = lst.download()
    refused(E_PARAM, lst.archive_encode)
    c255 = np.zeros(2, np.uint8)
    c255[1] = 255
    same_streams(lst.download(), kept)
    lst.set_host(np.zeros(2, np.uint8), np.arange(2, dtype=np.uint32), None, c255, np.full(255, 0x12, np.uint8), np.zeros(255, np.uint8))
    refused(E_PARAM, lst.archive_encode, False)
    assert lst.archive_encode(True)["archive"]["n_mismatches"] == 255          # (the fast level has one destination)
    lst.close()


# ------------------------------------------------------------------------------------------------ the assembly
def sets_with_count(seed, which, count, others=(11, 6)):
    """read sets whose set `which` has `count` reads (its mapping then has `count` entries in front of the guard)"""
    counts = [others[0], others[1], 4]
    counts[which] = count
    st = ru.state_with_counts(np.random.default_rng(seed), 30, True, counts)
    s = DividedReadsSets(30, True, False)
    s.append(ru.state_batch(st, 30, True))
    s.finish()
    return s


@pytest.mark.parametrize("path", PGASM_FIXTURES, ids=pgasm_name)
def test_from_assembly_equals_the_fixtures_and_the_host_mapping(path):
    fx = load_pgasm(path)
    L, symbols, R = int(fx["L"]), int(fx["symbols"]), fx["rows"].shape[0]
    asm = PgAssembler(device=0)
    lst = ReadsList(0)
    refused(E_STATE, lst.from_assembly, asm)                                 # no run
    host = asm.run(fx["rows"], fx["next_read"], fx["overlap"], L, symbols)
    lst.from_assembly(asm)
    got = lst.download()
    assert got["off"].dtype == np.uint8 and np.array_equal(got["off"], fx["off"]) and np.array_equal(got["org_idx"], fx["org_idx"])
    assert np.array_equal(got["off"], host["off"]) and got["last_pos"] == int(fx["pg_len"]) - L
    assert not got["rev_comp"].any() and not got["mis_cnt"].any() and got["mis_sym"].size == 0
    t = lst.timing()
    assert t["call"] == "download" and lst.info()["n_entries"] == R
    other = PgAssembler(device=0)
    for which in ("hq", "lq", "n"):
        w = ("hq", "lq", "n").index(which)
        sets = sets_with_count(R + w, w, R)
        mapping = sets.get_mapping(which)[:-1]
        assert mapping.size == R
        want = other.run(fx["rows"], fx["next_read"], fx["overlap"], L, symbols, index_mapping=mapping)
        lst.from_assembly(asm, sets, which)
        t = lst.timing()
        assert t["call"] == "from_assembly" and t["bytes_up"] == 0 and t["bytes_down"] == 0 and t["bytes_device_copy"] == 2 * R
        got = lst.download()
        assert np.array_equal(got["org_idx"], want["org_idx"]) and np.array_equal(got["off"], want["off"]), which
        # the refused combinations, each followed by the earlier content
        refused(E_STATE, lst.from_assembly, other, sets, which)              # that run has applied a host mapping
        if R > 1:
            small = sets_with_count(R + 7 + w, w, R - 1)
            refused(E_PARAM, lst.from_assembly, asm, small, which)           # an index beyond the mapping
            small.close()
        same_streams(lst.download(), got, ("after the refusals", which))
        sets.close()
    for x in (asm, other, lst):
        x.close()


# ------------------------------------------------------------------------------------------------ the pair order
@pytest.mark.parametrize("path", PAIRORDER_FIXTURES, ids=pairorder_name)
def test_pair_order_equals_the_fixtures_and_the_host_route(path):
    org, st, _, _, _ = load_pairorder(path)
    dec = PgRCDecoder(100, device=0)
    want = dec.compressReadsOrder(org, st["form"])
    assert_pairorder(want, st)
    parts = po.split_three(org, 5)
    lists = [simple_list(p) for p in parts]
    got = ReadsList.pair_order(lists, st["form"])
    assert_pairorder(got, st)
    first = lists[0]
    t = first.timing()
    assert t["call"] == "pair_order" and t["bytes_up"] == 0 and t["bytes_down"] == dec.pairorder_timing()["bytes_down"]
    # a list that is not there; one list alone
    assert_pairorder(ReadsList.pair_order([lists[0], None, simple_list(np.concatenate(parts[1:]))], st["form"]), st)
    assert_pairorder(ReadsList.pair_order([None, simple_list(org), None], st["form"]), st)
    # the refusals of pgrc_pairorder_encode leave the lists usable
    if org.size >= 4:
        dup = org.copy()
        dup[1] = dup[0]
        refused(E_PARAM, ReadsList.pair_order, [simple_list(dup)], st["form"])
        refused(E_PARAM, ReadsList.pair_order, [simple_list(org[:-1])], st["form"])
        refused(E_PARAM, ReadsList.pair_order, lists, 9)
        assert_pairorder(ReadsList.pair_order(lists, st["form"]), st)
    dec.close()


def test_pair_order_in_all_four_forms_on_a_generated_order():
    org = po.make_order(77, 5000, **po.DEFAULT_MIX)
    lists = [simple_list(p) for p in po.split_three(org, 3)]
    dec = PgRCDecoder(100, device=0)
    for form in po.FORMS:
        assert_pairorder(ReadsList.pair_order(lists, form), dec.compressReadsOrder(org, form))
    dec.close()


# ------------------------------------------------------------------------------------------------ the pair positions
def matcher_with_results(read_org_count, match_pos):
    """a matcher whose results are the given positions (pgrc_match_set_results): read_org_count reads of a small text"""
    n = max(int(read_org_count), 1)
    ctx = MatchContext(100, 38, 3, 0, "c", device=0)
    ctx.set_pg_ascii(np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(1).integers(0, 4, size=4000)])
    ctx.set_reads_ascii(np.full((n, 100), ord("A"), np.uint8))
    ctx.init_results()
    pos = np.full(n, rl.FILL, dtype=np.uint64)
    pos[: match_pos.size] = match_pos
    ctx.set_results(pos, np.zeros(n, np.uint8), np.where(pos == rl.FILL, 255, 0).astype(np.uint8))
    return ctx, pos


def run_setting(s, W, dec):
    lists = {k: (ReadsList(0) if s[k] is not None else None) for k in ("hq", "lq", "n")}
    for k, l in lists.items():
        if l is not None:
            l.set_host(s[k][0], s[k][1])
    ctx, pos = matcher_with_results(s["read_org"].size, s["match_pos"])
    ro = np.zeros(pos.size, np.uint32)
    ro[: s["read_org"].size] = s["read_org"]
    got = lists["hq"].pair_positions(s["T"], W, lists["lq"], lists["n"], s["hq_len"], s["lq_len"], ctx, ro)
    want_arr = rl.positions_of(s, rl.positions_numpy)
    assert_pairpos(got, dec.compressReadsPgPositions(want_arr, W))
    t = lists["hq"].timing()
    assert t["call"] == "pair_positions" and t["bytes_up"] == 4 * pos.size and t["bytes_down"] == dec.pairpos_timing()["bytes_down"]
    ctx.close()
    for l in lists.values():
        if l is not None:
            l.close()


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5, 6, 7])
def test_pair_positions_of_seeded_settings(seed):
    """(seeds divisible by three put the LQ list across 2^32; T = 2 and absent lists are among them)"""
    dec = PgRCDecoder(100, device=0)
    s = rl.make_setting(seed, T=2 if seed == 7 else None)
    assert np.array_equal(rl.positions_of(s, rl.positions_numpy), rl.positions_of(s, rl.positions_literal))
    run_setting(s, 8, dec)
    if int(rl.positions_of(s, rl.positions_numpy).max(initial=0)) < 2**32:
        run_setting(s, 4, dec)
    dec.close()


def test_pair_positions_with_a_matcher_run_and_three_lists():
    case = xu.export_case(seed=21, G=60_000, n=3000, L=100, n_with_n=60, dups=50)
    g = gpu_match("c", case["pg"], case["reads"], 38, 33, 0, n_nset=case["n_n"])
    ctx, mpos = g["ctx"], g["pos"]
    matched = np.flatnonzero(mpos != rl.FILL)
    assert 100 < matched.size < mpos.size
    rng = np.random.default_rng(5)
    sizes = [4001 + (matched.size + 1) % 2, 700, 300]               # T even
    T = matched.size + sum(sizes)
    perm = rng.permutation(T).astype(np.uint32)
    read_org = np.zeros(mpos.size, np.uint32)                       # (what an unmatched read carries is never looked at)
    read_org[matched] = perm[: matched.size]
    at = matched.size
    lists, host = [], []
    for n in sizes:
        off, org = rng.integers(0, 120, size=n).astype(np.uint8), perm[at: at + n]
        at += n
        lists.append(simple_list(org, off))
        host.append((off, org))
    hq_len, lq_len = case["pg"].size, int(host[1][0].sum()) + 100
    want_arr = rl.positions_numpy(T, host[0], host[1], host[2], hq_len, lq_len, read_org, mpos)
    assert np.array_equal(want_arr, rl.positions_literal(T, host[0], host[1], host[2], hq_len, lq_len, read_org, mpos))
    dec = PgRCDecoder(100, device=0)
    for W in (4, 8):
        got = lists[0].pair_positions(T, W, lists[1], lists[2], hq_len, lq_len, ctx, read_org)
        assert_pairpos(got, dec.compressReadsPgPositions(want_arr, W))
    # the refusals: an index written twice, one never written, an index of T, a position of 2^32 with four bytes
    org2 = host[2][1].copy()
    org2[0] = host[1][1][0]
    twice = simple_list(org2, host[2][0])
    refused(E_PARAM, lists[0].pair_positions, T, 8, lists[1], twice, hq_len, lq_len, ctx, read_org)
    refused(E_PARAM, lists[0].pair_positions, T, 8, lists[1], None, hq_len, lq_len, ctx, read_org)         # the N list's indexes are never written
    refused(E_PARAM, lists[0].pair_positions, T + 2, 8, lists[1], lists[2], hq_len, lq_len, ctx, read_org)
    refused(E_PARAM, lists[0].pair_positions, T - 2, 8, lists[1], lists[2], hq_len, lq_len, ctx, read_org)
    org3 = host[2][1].copy()
    org3[5] = T
    refused(E_PARAM, lists[0].pair_positions, T, 8, lists[1], simple_list(org3, host[2][0]), hq_len, lq_len, ctx, read_org)
    refused(E_PARAM, lists[0].pair_positions, T, 4, lists[1], lists[2], 2**32, lq_len, ctx, read_org)
    refused(E_PARAM, lists[0].pair_positions, T, 5, lists[1], lists[2], hq_len, lq_len, ctx, read_org)
    refused(E_PARAM, lists[0].pair_positions, T, 8, lists[1], lists[2], hq_len, lq_len, ctx, read_org[:-1].copy(), DividedReadsSets(100, True, False))
    # ... after which the lists hold what they held and the call works
    same_streams(lists[0].download(), {"off": host[0][0], "org_idx": host[0][1], "rev_comp": np.zeros(sizes[0], np.uint8), "mis_cnt": np.zeros(sizes[0], np.uint8),
                                       "mis_sym": np.zeros(0, np.uint8), "mis_rev_off": np.zeros(0, np.uint8), "last_pos": 0})
    assert_pairpos(lists[0].pair_positions(T, 8, lists[1], lists[2], hq_len, lq_len, ctx, read_org), dec.compressReadsPgPositions(want_arr, 8))
    dec.close()


@pytest.mark.parametrize("path", PAIRPOS_FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def test_pair_positions_reproduce_the_fixtures(path):
    """lists and matched reads constructed to yield the fixture's array: the positions below 2^32 in ascending order are the HQ
    list as long as the step fits an offset (16 bits), the ones from 2^32 on the LQ list at base hq_len = the smallest of them, and
    what a step leaves out is a matched read of the matcher"""
    arr, st, _, _ = load_pairpos(path)
    arr = arr.astype(np.uint64)
    T, W = arr.size, int(st["pos_width"])
    idx = np.argsort(arr, kind="stable")
    high = arr[arr >= np.uint64(2**32)]
    hq_len = int(high.min()) if high.size else 2**32
    chains, left = [], []
    for lo, hi, base in ((0, 2**32, 0), (2**32, 2**64, hq_len)):
        off, org, cur = [], [], base
        for i in idx[(arr[idx] >= np.uint64(lo)) & (arr[idx] <= np.uint64(hi - 1))]:
            step = int(arr[i]) - cur
            if step <= 65535:
                off.append(step)
                org.append(i)
                cur = int(arr[i])
            else:
                left.append(i)
        chains.append((np.array(off, np.uint16), np.array(org, np.uint32)))
    left = np.array(left, dtype=np.int64)
    if W == 8 and "above" in path:
        assert chains[1][1].size > 0 and int(arr.max()) >= 2**32
    hq, lq = simple_list(chains[0][1], chains[0][0]), simple_list(chains[1][1], chains[1][0])
    ctx, pos = matcher_with_results(left.size, arr[left])
    ro = np.zeros(pos.size, np.uint32)
    ro[: left.size] = left
    assert np.array_equal(rl.positions_literal(T, chains[0], chains[1], None, hq_len, 0, ro, pos), arr)
    got = hq.pair_positions(T, W, lq, None, hq_len, 0, ctx, ro)
    assert_pairpos(got, st)
    ctx.close()
    hq.close()
    lq.close()


# ------------------------------------------------------------------------------------------------ the chain
def test_chain_from_the_assembly_to_the_pair_order():
    """continues test_gpu_rsets.test_chain_without_a_row_crossing_the_link with the same 20 000 reads: every list stage on the
    resident route and on the host route made from the existing calls"""
    L = 100
    genome, reads, quals = chain_records(L=L)
    div = DividedPCLReadsSets(L, 0.05, True, True, False)
    div.divide(reads, quals)
    sets = DividedReadsSets(L, True, False)
    sets.append_divider(div)
    sets.finish()
    ovl, asm, host_asm = OverlapFinder(), PgAssembler(device=0), PgAssembler(device=0)
    sets.overlap("hq", ovl, 0.6)
    sets.move_by_overlap(ovl)
    # the HQ pseudogenome and its list, the indexes mapped from the read sets
    sets.overlap("hq", ovl, 0.6)
    hq = ReadsList(0)
    hq.from_overlap(ovl, asm, sets, "hq")
    assert asm.timing()["bytes_down"] == 0 and asm.timing()["bytes_up"] == 0
    up = [hq.timing()["bytes_up"]]
    hq_map = sets.get_mapping("hq")[:-1]
    want_asm = ovl.assemble(host_asm, index_mapping=hq_map)
    got = hq.download()
    assert np.array_equal(got["org_idx"], want_asm["org_idx"]) and np.array_equal(got["off"], want_asm["off"]) and want_asm["off"].max() < 256
    assert got["last_pos"] == asm.pg_len - L == host_asm.pg_len - L
    # the matcher on the assembled text, the LQ + N sum set handed over on the device
    ctx = MatchContext(L, 38, 3, 0, "c", device=0)
    ctx.set_pg_packed_device(asm.packed_device(), asm.pg_len)
    sets.to_matcher(ctx)
    ctx.init_results()
    ctx.run(True)
    pos = ctx.get_results()[0]
    n_matched = int((pos != rl.FILL).sum())
    assert 0 < n_matched < pos.size
    # the export: read indexes from the read sets, the order made on the device
    read_org = np.concatenate([sets.get_mapping("lq")[:-1], sets.get_mapping("n")[:-1]])
    want_exp = ctx.export_pg_order(None, want_asm["off"].astype(np.uint8), want_asm["org_idx"], None, read_org, False, True)
    hq.export_pg_order(ctx, None, None, sets, False, True)
    t = hq.timing()
    up.append(t["bytes_up"])
    assert t["bytes_down"] == 0
    same_streams(hq.download(), want_exp, "export")
    assert want_exp["org_idx"].size == want_asm["org_idx"].size + n_matched and want_exp["mis_sym"].size > 0
    # the archive form: one block, the only list bytes that come down
    arch = hq.archive_encode(False, False)
    t = hq.timing()
    up.append(t["bytes_up"])
    assert t["call"] == "archive_encode" and t["bytes_down"] == arch["block_bytes"] and arch["one_block"]
    dec = PgRCDecoder(L, device=0)
    la.assert_streams(arch["archive"], dec.list_archive_encode(want_exp["mis_cnt"], want_exp["mis_sym"], want_exp["mis_rev_off"]))
    assert np.array_equal(arch["off"], want_exp["off"]) and np.array_equal(arch["rev_comp"], want_exp["rev_comp"]) and arch["org_idx"] is None
    # the LQ and the N list of what the matcher left
    sets.remove_matched(ctx)
    info = sets.info()
    assert info["count"][1] > 0 and info["count"][2] > 0 and info["count"][1] + info["count"][2] == pos.size - n_matched
    rest, rest_want = [], []
    for which in ("lq", "n"):
        sets.overlap(which, ovl, 0.6)
        a, b = PgAssembler(device=0), PgAssembler(device=0)
        ovl.assemble(a)
        lst = ReadsList(0)
        if which == "lq":
            lst.from_assembly(a, sets, which)
        else:                                       # the same in one call, the assembly's copy of the list to the host left out
            numbers = lst.from_overlap(ovl, a, sets, which)
            assert a.timing()["bytes_down"] == 0 and numbers["pg_len"] == a.pg_len > 0
        up.append(lst.timing()["bytes_up"])
        want = ovl.assemble(b, index_mapping=sets.get_mapping(which)[:-1])
        assert which == "lq" or all(numbers[k] == want[k] for k in numbers)
        got = lst.download()
        assert np.array_equal(got["org_idx"], want["org_idx"]) and np.array_equal(got["off"], want["off"]), which
        small = lst.archive_encode(False, True)
        assert small["archive"] is None and np.array_equal(small["org_idx"], want["org_idx"]) and np.array_equal(small["off"], want["off"])
        rest.append(lst)
        rest_want.append(want["org_idx"])
        a.close()
        b.close()
    # the pair order over the three lists
    parts = [want_exp["org_idx"]] + rest_want
    assert sum(p.size for p in parts) == reads.shape[0] and np.array_equal(np.sort(np.concatenate(parts)), np.arange(reads.shape[0]))
    for form in po.FORMS:
        assert_pairorder(ReadsList.pair_order([hq] + rest, form), dec.compressReadsOrder(parts, form))
        up.append(hq.timing()["bytes_up"])
    assert up == [0] * len(up)
    for x in [hq, ctx, dec, ovl, asm, host_asm, sets, div] + rest:
        x.close()


# ------------------------------------------------------------------------------------------------ the list's own coding states
def archive_block(lst, fast=False, want_org=True):
    """pgrc_rlist_archive_encode itself -> (the block's bytes as they came down, its archive form)"""
    import ctypes as C
    from pgrc_amd import _lib
    from pgrc_amd.decode import _list_archive_dict
    a = _lib.RlistArchive()
    code = _lib.lib.pgrc_rlist_archive_encode(lst._h, int(fast), int(want_org), C.byref(a))
    assert code == 0, _lib.lib.pgrc_rlist_last_error(lst._h)
    try:
        assert a.off == a.block and lst.timing()["bytes_down"] == a.block_bytes
        return C.string_at(a.block, int(a.block_bytes)), _list_archive_dict(a.archive, a.block)
    finally:
        _lib.lib.pgrc_rlist_archive_free(C.byref(a))


def test_coding_states_of_a_list_neither_share_nor_clobber():
    """one list handle runs the archive form, the pair order, the pair positions and the archive form again, a decode context
    of its own codes the same data in between: the two archive blocks are the same bytes, and every coding gives what the
    decode context gives.  The sizes are the smallest that cross the archive tile (TILE + 1 entries) and the scan block
    (4097 pairs); the tile being 8192, the list with the mismatches holds all but one of the 8194 entries, the LQ list the
    last one and the N list none."""
    n, pairs, L = TILE + 1, 4097, 40
    T = 2 * pairs
    sizes = (n, T - n, 0)
    cnt, sym, rev_off = la.make_list(905, n, L)
    assert sym.size > n // 4 and T > n
    rng = np.random.default_rng(905)
    org = po.make_order(905, pairs, **po.DEFAULT_MIX)
    assert org.size == T
    parts = np.split(org, np.cumsum(sizes)[:-1])
    offs = [rng.integers(0, 250, size=k).astype(np.uint8) for k in sizes]
    hq = ReadsList(0)
    hq.set_host(offs[0], parts[0], (rng.random(n) < 0.5).astype(np.uint8), cnt, sym, rev_off)
    rest = [simple_list(parts[k], offs[k]) for k in (1, 2)]
    hq_len, lq_len = int(offs[0].sum()) + L, int(offs[1].sum()) + L
    want_pos = rl.positions_numpy(T, (offs[0], parts[0]), (offs[1], parts[1]), (offs[2], parts[2]), hq_len, lq_len)
    dec = PgRCDecoder(L, device=0)

    block1, arch1 = archive_block(hq)
    kept = hq.download()
    want_arch = dec.list_archive_encode(kept["mis_cnt"], kept["mis_sym"], kept["mis_rev_off"])
    la.assert_streams(arch1, want_arch)
    for form in po.FORMS:
        got = ReadsList.pair_order([hq] + rest, form)
        assert_pairorder(got, dec.compressReadsOrder(parts, form))
        assert hq.timing()["bytes_down"] == dec.pairorder_timing()["bytes_down"]
    for W in (4, 8):
        got = hq.pair_positions(T, W, rest[0], rest[1], hq_len, lq_len)
        assert_pairpos(got, dec.compressReadsPgPositions(want_pos, W))
        assert hq.timing()["bytes_down"] == dec.pairpos_timing()["bytes_down"]
    la.assert_streams(dec.list_archive_encode(cnt, sym, rev_off), want_arch)
    block2, arch2 = archive_block(hq)
    assert block1 == block2 and len(block1) >= 6 * n + 2 * sym.size
    la.assert_streams(arch2, want_arch)
    same_streams(hq.download(), kept, "the list after its codings")
    for x in [hq, dec] + rest:
        x.close()


def test_a_list_closes_unused_and_after_a_refusal():
    ReadsList(0).close()                                    # no call: no coding state has a buffer or an event
    lst = ReadsList(0)
    refused(E_STATE, lst.timing)
    refused(E_PARAM, lst.set_host, np.zeros(4, np.uint8), np.arange(4, dtype=np.uint32), None, np.ones(4, np.uint8), None, None)
    refused(E_PARAM, ReadsList.pair_order, [lst], 9)
    lst.close()
    lst.close()                                             # (a second close is nothing)
    again = simple_list(np.arange(6, dtype=np.uint32)[::-1])
    assert np.array_equal(again.download()["org_idx"], np.arange(6, dtype=np.uint32)[::-1])
    assert_pairorder(ReadsList.pair_order([again], po.IGNORE), po.compress_parallel(np.arange(6, dtype=np.uint32)[::-1], po.IGNORE))
    again.close()
