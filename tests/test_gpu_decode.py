"""The read rebuild on the device (include/pgrc_decode.h, pgrc_amd/decode.py): rows equal to decode_util's restatement of
the reference decoder's writers and to the ground truth -- the input reads -- over export streams made on the device and
over the reference-made streams of the committed fixtures; list shapes at the edges (no RC flags or mismatches, empty
lists, lists sized to the device scan's block of 4096 and past its carry round of 1 048 576 entries, text spans too large
for LDS, a joined text above 2^32 symbols), rows fetched in pieces, bad windows refused;
and a round trip match -> export -> rebuild at millions of reads."""
import time

import numpy as np
import pytest

import decode_util as du
import export_util as xu
from pgrc_amd import MatchContext, PgRCDecoder, PgrcMatchError, synth

pytestmark = pytest.mark.gpu


def add_lists(dec, lists):
    for lst in lists:
        dec.add_list(lst["n"], lst["text_base"], off=lst.get("off"), pos=lst.get("pos"), rev_comp=lst.get("rc"),
                     mis_cnt=lst.get("mis_cnt"), mis_sym=lst.get("mis_sym"), mis_off=lst.get("mis_off"),
                     mis_off_rev_coded=lst.get("rev_coded", True), mis_sym_form=lst.get("form", 0),
                     bases_order=lst.get("order"))


def decoder(dc, lists=None):
    dec = PgRCDecoder(dc["L"], device=0)
    dec.set_text(dc["text"])
    add_lists(dec, dc["lists"] if lists is None else lists)
    return dec


def device_job(seed, L, pair, G=150_000, n=6000, n_with_n=150):
    """an export case whose old list reaches the Pg end, matched and exported on the device"""
    case = du.close_list(xu.export_case(seed=seed, G=G, n=n, L=L, n_with_n=n_with_n, paired=pair, dups=100,
                                        list_gap=min(60, L)), seed=seed, even=pair)
    seed_len = 24 if L < 64 else 38
    ctx = MatchContext(L, seed_len, L // 3, 0, "c", device=0)
    ctx.set_pg_ascii(case["pg"])
    ctx.set_reads_ascii(case["reads"])
    ctx.init_results()
    ctx.run(True)
    pos, rc, mism, _, matched = ctx.get_results()
    assert matched > n // 2
    res = {"pos": pos, "rc": rc, "mism": mism}
    pg_st = ctx.export_pg_order(None, case["list_off"], case["list_org"], case["list_rc"], case["read_org"],
                                rev_compl_pair_file=pair)
    org_st = ctx.export_original_order(case["read_org"], case["total"], pair_file_mode=pair, rev_compl_pair_file=pair)
    ctx.close()
    return case, res, pg_st, org_st


def check_all_orders(dc, pair, sane=None):
    """device == restatement in SE (without the pair-file rule), PE and ORD; == ground truth (rows of sane entries)"""
    dec = decoder(dc)
    if not pair:
        se = dec.writeAllReadsInSEMode()
        assert np.array_equal(se, du.write_se(dc))
        truth = dc["truth"][dc["hq_org"]] if "hq_org" in dc else None
        if truth is not None:
            ok = np.ones(truth.shape[0], bool) if sane is None else sane
            assert np.array_equal(se[: truth.shape[0]][ok, :-1], truth[ok])
    f1, f2 = dec.writeAllReadsInPEMode(dc["rl_idx_order"], revComplPairFile=pair)
    w1, w2 = du.write_pe(dc, dc["rl_idx_order"], pair)
    assert np.array_equal(f1, w1) and np.array_equal(f2, w2)
    bad_rl = np.zeros(len(dc["rl_idx_order"]), bool)
    if sane is not None:
        bad_rl = np.isin(dc["rl_idx_order"], np.flatnonzero(~sane))
    for p, f in enumerate((f1, f2)):
        ok = ~bad_rl[p::2]
        assert np.array_equal(f[ok], du.truth_rows_pe(dc, p)[ok]), p
    dec.close()
    check_ord(dc, pair)


def check_ord(dc, pair):
    """ORD over the original-order lists: device == restatement == ground truth"""
    dec = decoder(dc, dc["ord_lists"])
    files = dec.writeAllReadsInORDMode(dc["org2pos"], singleReadsMode=not pair, revComplPairFile=pair)
    want = du.write_ord(dict(dc, lists=dc["ord_lists"]), dc["org2pos"], paired=pair, pair_file=pair)
    for p, (f, w) in enumerate(zip(files, want)):
        assert np.array_equal(f, w), p
        assert np.array_equal(f, du.truth_rows_ord(dc, dc["text"], p, pair)), p
    dec.close()


JOBS = [   # (L, pair-file rule, archive symbol form, two-byte offsets)
    (37, False, False, False),
    (100, True, True, False),
    (150, False, True, True),
    (150, True, False, False),
    (250, False, False, True),
]


@pytest.mark.parametrize("L,pair,archive,wide", JOBS)
def test_device_rows_equal_restatement_and_reads(L, pair, archive, wide):
    case, res, pg_st, org_st = device_job(40 + L + pair, L, pair)
    dc = du.decode_case(case, res, pg_st, org_st, pair=pair, wide=wide, archive=archive)
    dc["hq_org"] = pg_st["org_idx"].astype(np.int64)
    assert dc["lists"][0]["form"] == (0 if archive else 1) and pg_st["mis_cnt"].sum() > 100
    if archive and L == 100:
        assert dc["lists"][0]["order"] != b"ACGTN"       # (this job's mismatch counts reorder the symbols)
    check_all_orders(dc, pair)


@pytest.mark.parametrize("name", xu.EXPORT_GOLDEN)
def test_reference_made_streams_decode_to_the_reads(name):
    """the committed fixtures hold the compiled reference's own export streams: decoded, they give back the regenerated
    reads (in Pg order, matches beyond the old list's last entry carry offsets written from -1 -- see
    decode_util.close_list -- and are checked against the restatement only)"""
    case, pair, _, res, _, streams = xu.load_export_golden(name)
    pg_st, org_st = du.streams_from_bytes(streams["pg"]), du.streams_from_bytes(streams["org"])
    dc = du.decode_case(case, res, pg_st, org_st, pair=pair)
    dc["hq_org"] = pg_st["org_idx"].astype(np.int64)
    sane = du.sane_hq_entries(case, res, pg_st)
    assert sane.sum() > 1000
    if sane.all():
        check_all_orders(dc, pair)
        return
    # windows of the tail entries may reach past the text end (the reference would read beyond its string): SE over the
    # entries in front of them, ORD (positions from orgIdx2PgPos) over all
    k = int(np.argmin(sane))
    hq = dict(dc["lists"][0])
    nm = int(hq["mis_cnt"][:k].astype(np.int64).sum())
    for key in ("off", "rc", "mis_cnt"):
        hq[key] = hq[key][:k]
    hq["mis_sym"], hq["mis_off"], hq["n"] = hq["mis_sym"][:nm], hq["mis_off"][:nm], k
    head = dict(dc, lists=[hq])
    dec = decoder(head)
    se = dec.writeAllReadsInSEMode()
    dec.close()
    assert np.array_equal(se, du.write_se(head))
    if not pair:          # (under the pair-file rule, SE order does not orient the odd indexes' mismatch lists)
        assert np.array_equal(se[:, :-1], dc["truth"][dc["hq_org"][:k]])
    check_ord(dc, pair)


def _random_text(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)]


def test_lists_without_flags_or_mismatches_and_empty_lists():
    rng = np.random.default_rng(3)
    L = 100
    text = _random_text(rng, 50_000)
    text[rng.integers(0, text.size, 300)] = ord("N")
    hq = {"text_base": 0, "n": 400, "off": rng.integers(0, 100, 400).astype(np.uint8)}
    lq = {"text_base": 45_000, "n": 0, "off": np.zeros(0, np.uint8)}
    nl = {"text_base": 46_000, "n": 30, "pos": np.arange(30) * 7}
    dc = {"L": L, "text": text, "lists": [hq, lq, nl]}
    dec = decoder(dc)
    se = dec.writeAllReadsInSEMode()
    assert se.shape == (430, L + 1) and np.array_equal(se, du.write_se(dc))
    order = rng.permutation(430).astype(np.uint32)
    f1, f2 = dec.writeAllReadsInPEMode(order)
    w1, w2 = du.write_pe(dc, order, False)
    assert np.array_equal(f1, w1) and np.array_equal(f2, w2)
    dec.close()
    empty = PgRCDecoder(L, device=0)
    empty.set_text(text)
    empty.add_list(0, 0, off=np.zeros(0, np.uint8), rev_comp=np.zeros(0, np.uint8), mis_cnt=np.zeros(0, np.uint8),
                   mis_sym=np.zeros(0, np.uint8), mis_off=np.zeros(0, np.uint8))
    assert empty.writeAllReadsInSEMode().shape == (0, L + 1)
    assert [f.shape for f in empty.writeAllReadsInORDMode(np.zeros(0, np.uint64))] == [(0, L + 1)]


def _hq_with_mismatches(rng, n, L, pos, form):
    cnt = rng.integers(0, 4, n).astype(np.uint8)
    offs = np.concatenate([np.sort(rng.choice(L, size=c, replace=False)) for c in cnt]).astype(np.int64)
    m = offs.size
    if form == 1:
        sym = ((rng.integers(0, 4, m) << 4) | rng.integers(0, 5, m)).astype(np.uint8)
    else:
        sym = rng.integers(0, 4, m).astype(np.uint8)
    return {"text_base": 0, "n": n, "pos": pos, "rc": (rng.random(n) < 0.5).astype(np.uint8), "mis_cnt": cnt,
            "mis_sym": sym, "mis_off": du.offsets_to_rev_offsets(cnt, offs, L).astype(np.uint8), "rev_coded": True,
            "form": form, "order": b"TGNAC" if form == 0 else None}


def _mismatch_streams(rng, n, L):
    """0..3 mismatches per entry at distinct ascending offsets, without a loop over the entries -> (mis_cnt, the offsets in
    list order, the rev-coded offsets as the stream holds them: per entry L-1 - off[m-1], then off[i+1] - 1 - off[i] downwards)"""
    cnt = rng.integers(0, 4, n).astype(np.uint8)
    have = np.arange(3)[None, :] < cnt[:, None]
    pick = np.argsort(rng.random((n, L)), axis=1)[:, :3]                # three distinct offsets per entry
    asc = np.sort(np.where(have, pick, L), axis=1)                      # the entry's own come first, ascending
    desc = np.take_along_axis(asc, np.maximum(cnt[:, None].astype(np.int64) - 1 - np.arange(3)[None, :], 0), axis=1)
    above = np.concatenate([np.full((n, 1), L), desc[:, :-1]], axis=1)  # what the walk stands behind: L, then the last offset
    return cnt, asc[have].astype(np.int64), (above - 1 - desc)[have].astype(np.int64)


def _scan_edge_job(seed, n_hq, n_lq, T, lq_type, form, L=16):
    """Hand-made lists that drive the decoder's three scans at given sizes: an HQ list at delta offsets with RC flags and
    mismatches (the `mcum` scan and its total), an LQ list at delta offsets of `lq_type` behind a non-zero text_base (the
    positions scan with a start), and T ORD positions on both sides of hqPgLen (the rank scan).  Offsets of 0..3 keep the
    text at about 1.5 symbols per entry; the u16 list has some above 255."""
    rng = np.random.default_rng(seed)
    hq_off = rng.integers(0, 4, n_hq).astype(np.uint8)
    hq_len = int(hq_off.sum(dtype=np.int64)) + L            # an HQ text ends where its last read ends
    lq_off = rng.integers(0, 4, n_lq).astype(lq_type)
    if lq_type is np.uint16:
        lq_off[rng.integers(0, n_lq, 1 + n_lq // 1000)] = rng.integers(256, 1000, 1 + n_lq // 1000)
    text = _random_text(rng, hq_len + int(lq_off.sum(dtype=np.int64)) + L)
    cnt, offs, rev = _mismatch_streams(rng, n_hq, L)
    assert np.array_equal(du.rev_offsets_to_offsets(cnt, rev, L), offs)
    if n_hq <= 5000:
        assert np.array_equal(du.offsets_to_rev_offsets(cnt, offs, L), rev)
    m = offs.size
    sym = ((rng.integers(0, 4, m) << 4) | rng.integers(0, 5, m)).astype(np.uint8) if form == 1 else rng.integers(0, 4, m).astype(np.uint8)
    hq = {"text_base": 0, "n": n_hq, "off": hq_off, "rc": (rng.random(n_hq) < 0.5).astype(np.uint8), "mis_cnt": cnt,
          "mis_sym": sym, "mis_off": rev.astype(np.uint8), "rev_coded": True, "form": form,
          "order": b"TGNAC" if form == 0 else None}
    lq = {"text_base": hq_len, "n": n_lq, "off": lq_off}
    below = rng.random(T) < 0.5                              # about T / 2 rows below hqPgLen: never more than HQ entries
    o2p = np.where(below, rng.integers(0, hq_len - L + 1, T), rng.integers(hq_len, text.size - L + 1, T)).astype(np.uint64)
    assert 0 < hq_len and int(below.sum()) <= n_hq
    return {"L": L, "text": text, "lists": [hq, lq]}, o2p


def _check_scan_edge_job(dc, o2p):
    dec = decoder(dc)
    se = dec.writeAllReadsInSEMode()
    assert se.shape == (dc["lists"][0]["n"] + dc["lists"][1]["n"], dc["L"] + 1)
    assert np.array_equal(se, du.write_se(dc))
    (rows,) = dec.writeAllReadsInORDMode(o2p)
    assert rows.shape == (o2p.size, dc["L"] + 1)
    assert np.array_equal(rows, du.write_ord(dc, o2p, False, False)[0])
    dec.close()


@pytest.mark.parametrize("lq_type,form", [(np.uint8, 1), (np.uint16, 0)])
@pytest.mark.parametrize("n", [1, 4095, 4096, 4097])
def test_lists_at_the_scan_block_edges(n, lq_type, form):
    """n entries per list and T = n ORD rows around the device scan's block of 4096: the positions scan starts from a
    text_base other than 0, the mismatch list starts end in their total, the ranks of the HQ rows in theirs"""
    dc, o2p = _scan_edge_job(100 + n, n, n, n, lq_type, form)
    assert dc["lists"][1]["text_base"] > 0
    _check_scan_edge_job(dc, o2p)


def test_lists_past_one_carry_round_of_the_scan():
    """1 048 577 LQ entries at u16 offsets behind a non-zero text_base, an HQ list with mismatches that also crosses
    1 048 576 entries, and as many ORD rows: the scans' carry kernel goes into its second round of 256 blocks"""
    n = (1 << 20) + 1
    dc, o2p = _scan_edge_job(7, n + 22, n, n, np.uint16, 1)
    assert dc["lists"][1]["text_base"] > 0 and dc["lists"][0]["mis_cnt"].sum(dtype=np.int64) > n
    _check_scan_edge_job(dc, o2p)


def test_tile_span_too_large_for_lds_takes_the_gathers():
    """SE rows whose windows lie far apart (a tile's span above the LDS bound): the per-row gathers"""
    rng = np.random.default_rng(4)
    L = 150
    text = _random_text(rng, 3_000_000)
    n = 2500
    pos = np.sort(rng.choice(text.size - L, size=n, replace=False))       # ~1200 apart: spans of ~80 KB per tile
    for form in (0, 1):
        dc = {"L": L, "text": text, "lists": [_hq_with_mismatches(rng, n, L, pos, form)]}
        dec = decoder(dc)
        assert np.array_equal(dec.writeAllReadsInSEMode(), du.write_se(dc))
        dec.close()


def test_rows_in_pieces_equal_one_fetch():
    import torch
    case, res, pg_st, org_st = device_job(77, 150, False)
    dc = du.decode_case(case, res, pg_st, org_st, pair=False)
    dec = decoder(dc)
    dec.set_order(1, len(dc["rl_idx_order"]), rl_idx_order=dc["rl_idx_order"])      # PE
    n = dec.row_count(1)
    whole = dec.rows(1)
    cuts = [0, 1, 63, 64, 1000, n - 7, n]
    parts = [dec.rows(1, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts), whole)
    pinned = torch.empty(n * 151, dtype=torch.uint8, pin_memory=True)          # written by the copy engine directly
    got = dec.rows(1, 0, n, out=pinned.numpy().reshape(n, 151))
    assert np.array_equal(got, whole)
    with pytest.raises(PgrcMatchError) as e:
        dec.rows(1, n - 2, 3)
    assert e.value.code == 1
    dec.close()


def test_windows_past_the_text_end_are_param_errors():
    rng = np.random.default_rng(6)
    L = 100
    text = _random_text(rng, 10_000)
    dec = PgRCDecoder(L, device=0)
    dec.set_text(text)
    with pytest.raises(PgrcMatchError) as e:
        dec.add_list(3, 0, pos=np.array([0, 5, text.size - L + 1]))
    assert e.value.code == 1 and "past the text end" in str(e.value)
    with pytest.raises(PgrcMatchError) as e:
        dec.add_list(2, 9_900, off=np.array([0, 1], np.uint8))                 # text_base + offsets past the end
    assert e.value.code == 1
    dec.add_list(3, 0, pos=np.array([0, 5, text.size - L]))                     # the last window ends at the text end
    assert dec.writeAllReadsInSEMode()[2, :-1].tobytes() == text[-L:].tobytes()
    with pytest.raises(PgrcMatchError) as e:
        dec.writeAllReadsInORDMode(np.array([0, text.size - L + 1, 3], np.uint64))
    assert e.value.code == 1
    with pytest.raises(PgrcMatchError) as e:
        dec.writeAllReadsInPEMode(np.array([0, 1, 3], np.uint32))
    assert e.value.code == 1
    dec.close()


def test_joined_text_above_4g_symbols():
    """positions are 64-bit (isJoinedPgLengthStd == false): a sparse list near the end of a 2^32 + 3000-symbol text"""
    rng = np.random.default_rng(8)
    L = 150
    size = (1 << 32) + 3000
    text = np.zeros(size, np.uint8)                       # (untouched pages stay unallocated on the host)
    tail = size - 40_000
    text[tail:] = _random_text(rng, size - tail)
    n = 300
    pos = np.sort(tail + rng.choice(size - tail - L + 1, size=n, replace=False)).astype(np.uint64)
    pos[-1] = size - L
    lst = _hq_with_mismatches(rng, n, L, pos, 0)
    dec = PgRCDecoder(L, device=0)
    dec.set_text(text)
    add_lists(dec, [lst])
    got = dec.writeAllReadsInSEMode()
    want = du.hq_rows(text, L, pos.astype(np.int64), lst["rc"].astype(bool), lst, np.arange(n))
    assert np.array_equal(got[:, :-1], want)
    o2p = pos[::-1].copy()              # ORD: row i takes HQ entry i (its flags and mismatches) at its own position
    files = dec.writeAllReadsInORDMode(o2p)
    assert np.array_equal(files[0], du.write_ord({"L": L, "text": text, "lists": [lst]}, o2p, False, False)[0])
    dec.close()


def test_round_trip_at_scale():
    """4 M reads x 150 bp over 80 Mbp: MatchContext -> export (Pg order with the order made on the device; original
    order) -> rebuild; every SE row is its read, every ORD row the read of its original index"""
    t0 = time.time()
    L, G, n = 150, 80_000_000, 4_000_000
    g = synth.pg_params(G, seed=11, tandem_every=4)
    pg = synth.pg_host(g)
    reads = synth.reads_host(g, pg, synth.reads_params(n, L, seed=11, n_with_n=20_000))
    # the old list: entries every 200 symbols up to G - L (an HQ list reaches the Pg end)
    lpos = np.arange(0, G - L + 1, 200, dtype=np.int64)
    if lpos[-1] != G - L:
        lpos = np.append(lpos, G - L)
    loff = np.diff(lpos, prepend=0).astype(np.uint8)
    h = lpos.size
    lorg = (n + np.arange(h)).astype(np.uint32)
    ctx = MatchContext(L, 38, 50, 0, "c", device=0)
    ctx.set_pg_ascii(pg)
    ctx.set_reads_ascii(reads)
    ctx.init_results()
    ctx.run(True)
    pos, rc, mism, _, matched = ctx.get_results()
    assert matched > n // 2
    st = ctx.export_pg_order(None, loff, lorg)
    ost = ctx.export_original_order(np.arange(n, dtype=np.uint32), n + h)
    ctx.close()
    um = np.flatnonzero(mism == 255)
    text = np.concatenate([pg, reads[um].reshape(-1)])
    dec = PgRCDecoder(L, device=0)
    dec.set_text(text)
    hq = {"text_base": 0, "n": st["org_idx"].size, "off": st["off"], "rc": st["rev_comp"], "mis_cnt": st["mis_cnt"],
          "mis_sym": st["mis_sym"], "mis_off": st["mis_rev_off"], "form": 1}
    lq = {"text_base": G, "n": um.size, "pos": np.arange(um.size, dtype=np.uint64) * L}
    add_lists(dec, [hq, lq])
    se = dec.writeAllReadsInSEMode()
    org = st["org_idx"].astype(np.int64)
    r = org < n
    assert r.sum() == matched
    assert np.array_equal(se[: org.size][r, :-1], reads[org[r]])
    assert np.array_equal(se[org.size:, :-1], reads[um])
    assert (se[:, -1] == ord("\n")).all()
    # ORD: one row per original index; fillers (the old list's indexes) at position 0
    o2p = np.zeros(n + h, np.uint64)
    o2p[:n][mism != 255] = pos[mism != 255]
    o2p[um] = G + np.arange(um.size, dtype=np.uint64) * L
    dec2 = PgRCDecoder(L, device=0)
    dec2.set_text(text)
    add_lists(dec2, [{"text_base": 0, "n": ost["org_idx"].size, "rc": ost["rev_comp"], "mis_cnt": ost["mis_cnt"],
                      "mis_sym": ost["mis_sym"], "mis_off": ost["mis_rev_off"], "form": 1}, lq])
    (rows,) = dec2.writeAllReadsInORDMode(o2p)
    assert np.array_equal(rows[:n, :-1], reads)
    assert (rows[n:, :-1] == pg[:L]).all()
    dec.close()
    dec2.close()
    assert time.time() - t0 < 120
