"""The restore of the matched pseudogenomes on the device (pgrc_decode_set_mapped_text, PgRCDecoder.restoreMatchedPgs):
the device text equals tests/pgmap_util's literal restatement of restoreMatchedPg and the original texts, over the
reference-made fixtures, over matches made on the device and mapped by the restatement of markAndRemoveExactMatches,
over hand-made chains (deep, fan-in), over the hop-class rule for bytes c(c(x)) does not return, with 8-byte offsets
above 2^32 HQ symbols, with empty parts; malformed input is refused with PGRC_E_PARAM and leaves no text; and the
rebuild of the reads after the restore equals the rebuild after set_text of the original text."""
import os

import numpy as np
import pytest

import decode_util as du
import pgmap_util as pu
from pgrc_amd import CopMEMMatcher, MatchContext, PgRCDecoder, PgrcMatchError, synth
from test_gpu_decode import add_lists, device_job
from test_pgmap_oracle import FIXTURES, load_case

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = 1, 6


def device_matches(hq, target_len):
    tm = CopMEMMatcher(hq, target_len, device=0)
    return lambda src, q, dis, rc: tm.matchTexts(q, dis, rc)


def restore(mapped, lens, org_hq_len, offs, lns, rev_compl=True, L=100):
    dec = PgRCDecoder(L, device=0)
    dec.restoreMatchedPgs(mapped, lens, org_hq_len, offs, lns, rev_compl)
    return dec


def check_restore(mapped, lens, org_hq_len, offs, lns, rev_compl=True, originals=None):
    want = pu.restore_matched_pgs(mapped, lens, org_hq_len, offs, lns, rev_compl)
    dec = restore(mapped, lens, org_hq_len, offs, lns, rev_compl)
    assert dec.text_lengths() == tuple(len(w) for w in want)
    got = dec.text().tobytes()
    assert got == b"".join(want)
    if originals is not None:
        assert got == b"".join(np.asarray(t, np.uint8).tobytes() for t in originals)
    t = dec.restore_timing()
    dec.close()
    return t


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[6:-4])
def test_reference_fixtures_restore_to_the_texts(path):
    z, texts, _ = load_case(path)
    mapped = b"".join(z[f"mapped{p}"].tobytes() for p in range(3))
    lens = [z[f"mapped{p}"].size for p in range(3)]
    offs = [z[f"off{p}"].tobytes() for p in range(3)]
    lns = [z[f"len{p}"].tobytes() for p in range(3)]
    if not lens[2]:                                     # an empty N part: its streams are not stored
        offs[2], lns[2] = b"", b""
    t = check_restore(mapped, lens, texts[0].size, offs, lns, originals=texts)
    assert t["marks"] == [int((z[f"mapped{p}"] == pu.MATCH_MARK).sum()) for p in range(3)]


@pytest.mark.parametrize("G", [20_000, 300_000, 2_000_000])
@pytest.mark.parametrize("rev_compl", [True, False])
def test_device_made_matches(G, rev_compl):
    hq, lq, nn = pu.make_texts(900 + G // 1000, G, G // 3, G // 10, nrep=G // 2000, chains=4, chain_depth=4)
    tl = 40
    mapped, lens, offs, lns, found = pu.map_all(hq, lq, nn, device_matches(hq, tl), tl, rev_compl)
    assert sum(int(f.shape[0]) for f in found) > 10
    if pu.hq_sources_valid(mapped[:lens[0]], offs[0], lns[0], hq.size):
        t = check_restore(mapped, lens, hq.size, offs, lns, rev_compl, originals=(hq, lq, nn))
        assert t["marks"][0] > 0 and t["matched"][0] > 0
    else:
        # a forward self-copy that overlaps its destination: the reference would clip it; the device refuses it
        assert not rev_compl
        dec = PgRCDecoder(100, device=0)
        with pytest.raises(PgrcMatchError) as e:
            dec.restoreMatchedPgs(mapped, lens, hq.size, offs, lns, rev_compl)
        assert e.value.code == E_PARAM
        dec.close()


def _random(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n).tobytes()


def test_deep_chain_resolves_in_logarithmic_passes():
    rng = np.random.default_rng(3)
    W, depth = 64, 4096
    pieces = [_random(rng, W)] + [(W * i, W) for i in range(depth)]      # mark i copies mark i-1 (the literal for i=0)
    hm, ho, hl = pu.build_part(pieces, min_len=20)
    lm, lo, ll = pu.build_part([b"AC", (W * depth, W), b"GT"], min_len=20)  # LQ: the deepest HQ match, one hop more
    mapped, lens, offs, lns = pu.join_parts([(hm, ho, hl), (lm, lo, ll), (b"", b"", b"")])
    t = check_restore(mapped, lens, W * (depth + 1), offs, lns)
    assert t["marks"] == [depth, 1, 0]
    assert t["passes"] <= 14                            # ceil(log2(4096)) + 2


def test_fan_in_from_one_match():
    rng = np.random.default_rng(4)
    lit = _random(rng, 500)
    pieces = [lit, (10, 300)]                           # the hub: output [500, 800)
    for i in range(3000):
        pieces += [_random(rng, 1 + i % 7), (500 + (i % 200), 50 + i % 50)]
    hm, ho, hl = pu.build_part(pieces, min_len=50)
    hq = pu.restore_matched_pg(b"", 10**6, hm, ho, hl, True, True)
    lm, lo, ll = pu.build_part([(550, 120), b"N", (600, 60)], min_len=50)
    mapped, lens, offs, lns = pu.join_parts([(hm, ho, hl), (lm, lo, ll), (b"", b"", b"")])
    check_restore(mapped, lens, len(hq), offs, lns)


@pytest.mark.parametrize("rev_compl", [True, False])
def test_hop_classes(rev_compl):
    """bytes reached through 0, 1, 2 and 3 hops: c(x), then c(c(x)) -- not x -- for lower case, U, IUPAC and bytes
    outside complementsLut"""
    lit = b"acgtuRYkmbdhvnN#\x00\xff" + bytes(range(0x61, 0x7b))
    n = len(lit)
    pieces = [lit, (0, n), b"ACGT", (n, n), (2 * n + 4, n), (5, 7)]     # 1, 2 and 3 hops from lit
    hm, ho, hl = pu.build_part(pieces, min_len=0)
    hq = pu.restore_matched_pg(b"", 10**6, hm, ho, hl, rev_compl, True)
    lm, lo, ll = pu.build_part([(2 * n + 4, n), b"n", (3 * n + 4, n)], min_len=3)
    mapped, lens, offs, lns = pu.join_parts([(hm, ho, hl), (lm, lo, ll), (b"", b"", b"")])
    check_restore(mapped, lens, len(hq), offs, lns, rev_compl)
    if rev_compl:
        two = pu.reverse_complement(pu.reverse_complement(lit))
        assert hq[2 * n + 4: 3 * n + 4] == two and two != lit


def test_eight_byte_offsets_above_4g_symbols():
    """org_hq_len > 2^32: 8-byte offsets; a sparse HQ (zeros, then a random tail with marks sourcing from the tail)"""
    rng = np.random.default_rng(8)
    size = (1 << 32) + 3000
    tail = size - 60_000
    t = bytearray(_random(rng, size - tail))
    marks = []                                         # (dest, src, len) in tail coordinates, src + len <= dest
    for d in range(6000, 58_000, 4000):
        s, L = int(rng.integers(0, d - 500)), int(rng.integers(60, 400))
        L = min(L, d - s)
        t[d:d + L] = pu.reverse_complement(bytes(t[s:s + L]))
        marks.append((d, s, L))
    pieces, at = [], 0
    for d, s, L in marks:
        pieces += [bytes(t[at:d]), (tail + s, L)]
        at = d + L
    pieces.append(bytes(t[at:]))
    hm, ho, hl = pu.build_part(pieces, min_len=45, width=8)
    lm, lo, ll = pu.build_part([b"ACGT", (tail + 100, 70), b"TTT"], min_len=45, width=8)
    mapped = np.zeros(tail + len(hm) + len(lm), np.uint8)      # (untouched pages stay unallocated on the host)
    mapped[tail:tail + len(hm)] = np.frombuffer(hm, np.uint8)
    mapped[tail + len(hm):] = np.frombuffer(lm, np.uint8)
    dec = PgRCDecoder(100, device=0)
    dec.restoreMatchedPgs(mapped, [tail + len(hm), len(lm), 0], size, [ho, lo, b""], [hl, ll, b""])
    assert dec.text_lengths() == (size, 4 + 70 + 3, 0)
    assert dec.text(tail, size - tail).tobytes() == bytes(t)
    assert not dec.text(0, 1 << 20).any() and not dec.text(tail - (1 << 20), 1 << 20).any()
    assert dec.text(size, 77).tobytes() == b"ACGT" + pu.reverse_complement(bytes(t[100:170])) + b"TTT"
    assert dec.restore_timing()["marks"] == [len(marks), 1, 0]
    dec.close()


def test_empty_parts_and_no_marks():
    rng = np.random.default_rng(5)
    hq = _random(rng, 5000)
    for parts in ([(hq, b"", b""), (b"", b"", b""), (b"", b"", b"")],              # no matcher (streams empty)
                  [(hq, b"", bytes([45])), (b"", b"", bytes([45])), (b"", b"", b"")],   # empty LQ, streams hold min only
                  [(hq, b"", bytes([45])), (b"ACGTN", b"", bytes([45])), (b"NNNN", b"", bytes([45]))]):
        mapped, lens, offs, lns = pu.join_parts(parts)
        t = check_restore(mapped, lens, len(hq), offs, lns)
        assert t["marks"] == [0, 0, 0] and t["passes"] == 0
    mapped, lens, offs, lns = pu.join_parts([(b"", b"", b"")] * 3)
    check_restore(mapped, lens, 0, offs, lns)


def _malformed():
    rng = np.random.default_rng(6)
    lit = _random(rng, 400)
    good_h = pu.build_part([lit, (10, 60)], min_len=45)
    good_l = pu.build_part([b"AC", (20, 50)], min_len=45)
    n_hq = 460
    hm, ho, hl = good_h
    lm, lo, ll = good_l
    yield "marks differ from values", [(hm + b"%", ho, hl), good_l], n_hq
    yield "values without marks", [(hm, ho, hl + b"\x00"), good_l], n_hq
    yield "value past the stream end", [(hm, ho, hl[:-1] + bytes([hl[-1] | 0x80])), good_l], n_hq
    yield "value longer than 10 bytes", [(hm, ho, hl[:1] + b"\x80" * 10 + b"\x01"), good_l], n_hq
    yield "offsets stream too long", [(hm, ho + b"\x00", hl), good_l], n_hq
    yield "offsets stream too short", [(hm, ho[:-1], hl), good_l], n_hq
    yield "LQ source past the HQ end", [good_h, pu.build_part([b"AC", (n_hq - 49, 50)], min_len=45)], n_hq
    yield "HQ source reaches its output", [pu.build_part([lit, (351, 50)], min_len=45), good_l], 450
    yield "HQ forward overlap", [pu.build_part([lit, (380, 60)], min_len=45), good_l], n_hq
    yield "HQ source past its end", [pu.build_part([lit, (2**32 - 10, 60)], min_len=45), good_l], n_hq
    yield "restored HQ length", [good_h, good_l], n_hq + 1


@pytest.mark.parametrize("case", list(_malformed()), ids=lambda c: c[0])
def test_malformed_input_is_refused(case):
    _, parts, org = case
    mapped, lens, offs, lns = pu.join_parts(parts + [(b"", b"", b"")])
    dec = PgRCDecoder(50, device=0)
    dec.set_text(np.frombuffer(b"ACGT" * 100, np.uint8))
    with pytest.raises(PgrcMatchError) as e:
        dec.restoreMatchedPgs(mapped, lens, org, offs, lns)
    assert e.value.code == E_PARAM
    with pytest.raises(PgrcMatchError) as e:                # no text afterwards
        dec.add_list(1, 0, pos=np.zeros(1, np.uint64))
    assert e.value.code == E_STATE
    with pytest.raises(PgrcMatchError):
        dec.text_lengths()
    # the same context restores well-formed input afterwards
    good = pu.join_parts([(b"ACGT" * 20, b"", b""), (b"", b"", b""), (b"", b"", b"")])
    dec.restoreMatchedPgs(*good[:2], 80, *good[2:])
    assert dec.text().tobytes() == b"ACGT" * 20
    dec.close()


def _rows(dec, dc, pair):
    """SE (without the pair-file rule), PE and ORD rows of the job after the text is installed"""
    out = []
    add_lists(dec, dc["lists"])
    if not pair:
        out.append(dec.writeAllReadsInSEMode())
    out += list(dec.writeAllReadsInPEMode(dc["rl_idx_order"], revComplPairFile=pair))
    return out


def _ord_rows(dec, dc, pair):
    add_lists(dec, dc["ord_lists"])
    return list(dec.writeAllReadsInORDMode(dc["org2pos"], singleReadsMode=not pair, revComplPairFile=pair))


@pytest.mark.parametrize("L,pair", [(100, False), (150, True)])
def test_rebuild_after_restore_equals_rebuild_after_set_text(L, pair):
    case, res, pg_st, org_st = device_job(70 + L, L, pair)
    dc = du.decode_case(case, res, pg_st, org_st, pair=pair)
    text = dc["text"].copy()
    hq_len = dc["lists"][1]["text_base"]
    lq_len = dc["lists"][2]["text_base"] - hq_len
    rng = np.random.default_rng(L)
    for _ in range(60):         # reverse-complement copies of HQ stretches in all three parts (both decoders get them)
        ln = int(rng.integers(50, 400))
        s, d = int(rng.integers(0, hq_len - ln)), int(rng.integers(0, text.size - ln))
        text[d:d + ln] = pu.revcomp_np(text[s:s + ln])
    dc["text"] = text
    hq, lq, nn = text[:hq_len], text[hq_len:hq_len + lq_len], text[hq_len + lq_len:]
    mapped, lens, offs, lns, found = pu.map_all(hq, lq, nn, device_matches(hq, 36), 36)
    assert found[0].shape[0] > 0 and found[1].shape[0] > 0
    a, b = PgRCDecoder(L, device=0), PgRCDecoder(L, device=0)
    a.restoreMatchedPgs(mapped, lens, hq.size, offs, lns)
    assert a.text_lengths() == (hq.size, lq.size, nn.size)
    b.set_text(text)
    for got, want in zip(_rows(a, dc, pair), _rows(b, dc, pair)):
        assert np.array_equal(got, want)
    a.restoreMatchedPgs(mapped, lens, hq.size, offs, lns)      # (the lists and the order were dropped)
    b.set_text(text)
    for got, want in zip(_ord_rows(a, dc, pair), _ord_rows(b, dc, pair)):
        assert np.array_equal(got, want)
    a.close()
    b.close()


def test_round_trip_at_scale():
    """1 M reads x 150 bp over a 20 Mbp HQ that carries reverse-complement copies (some of copies): match and export on
    the device, the pseudogenomes mapped from device-made Pg-vs-Pg matches, restored on the device, then rebuilt; every
    row is its read"""
    L, G, n = 150, 20_000_000, 1_000_000
    g = synth.pg_params(G, seed=21, tandem_every=4)
    pg = synth.pg_host(g)
    rng = np.random.default_rng(21)
    for _ in range(300):                                # RC copies, then copies of those copies
        ln = int(rng.integers(200, 5000))
        s = int(rng.integers(0, G // 2 - ln))
        d = int(rng.integers(G // 2, G - 2 * ln))
        pg[d:d + ln] = pu.revcomp_np(pg[s:s + ln])
        d2 = int(rng.integers(d + ln, G - ln))
        pg[d2:d2 + ln] = pu.revcomp_np(pg[d:d + ln])
    reads = synth.reads_host(g, pg, synth.reads_params(n, L, seed=21, n_with_n=5_000))
    ctx = MatchContext(L, 38, 50, 0, "c", device=0)
    ctx.set_pg_ascii(pg)
    ctx.set_reads_ascii(reads)
    ctx.init_results()
    ctx.run(True)
    _, _, mism, _, matched = ctx.get_results()
    assert matched > n // 2
    lpos = np.arange(0, G - L + 1, 200, dtype=np.int64)      # an old list up to the Pg end, as test_gpu_decode's
    lpos = np.append(lpos, G - L) if lpos[-1] != G - L else lpos
    st = ctx.export_pg_order(None, np.diff(lpos, prepend=0).astype(np.uint8), (n + np.arange(lpos.size)).astype(np.uint32))
    ctx.close()
    um = np.flatnonzero(mism == 255)
    lq = reads[um].reshape(-1)
    mapped, lens, offs, lns, found = pu.map_all(pg, lq, np.zeros(0, np.uint8), device_matches(pg, 45), 45)
    assert found[0].shape[0] > 300
    dec = PgRCDecoder(L, device=0)
    dec.restoreMatchedPgs(mapped, lens, G, offs, lns)
    assert dec.text_lengths() == (G, lq.size, 0)
    t = dec.restore_timing()
    assert t["marks"][0] > 300 and t["passes"] >= 2
    hq = {"text_base": 0, "n": st["org_idx"].size, "off": st["off"], "rc": st["rev_comp"], "mis_cnt": st["mis_cnt"],
          "mis_sym": st["mis_sym"], "mis_off": st["mis_rev_off"], "form": 1}
    lql = {"text_base": G, "n": um.size, "pos": np.arange(um.size, dtype=np.uint64) * L}
    add_lists(dec, [hq, lql])
    se = dec.writeAllReadsInSEMode()
    org = st["org_idx"].astype(np.int64)
    r = org < n
    assert r.sum() == matched
    assert np.array_equal(se[: org.size][r, :-1], reads[org[r]])
    assert np.array_equal(se[: org.size][~r, :-1], pg[lpos[:, None] + np.arange(L)][org[~r] - n])
    assert np.array_equal(se[org.size:, :-1], reads[um])
    dec.close()
