"""markAndRemoveExactMatches on the device (pgrc_mem_mark_and_remove, pgmap.hip): the mapped text and both streams, byte
for byte, against the reference-made fixtures and against tests/pgmap_util.mark_and_remove -- over the fixtures' matches and
the device's own, through the device's restore (which shares no code with the mapping) back to the original texts, over
hand-made match lists at the scan and block edges (the mapping does not look at symbols, so these need not be real matches),
at the text kernel's edges, with every width of both streams (8-byte offsets over a source above 2^32 symbols), on a text shorter than K, and over every malformed input of the header.  Every test
runs matchTexts first, so that the destination is resident."""
import ctypes as C
import os

import numpy as np
import pytest

import pgmap_util as pu
from pgrc_amd import CopMEMMatcher, PgRCDecoder, PgrcMatchError, _lib
from test_pgmap_oracle import FIXTURES, load_case

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = 1, 6
ACGT = np.frombuffer(b"ACGT", np.uint8)
MAPPABLE = [f for f in FIXTURES if int(np.load(f)["params"][1]) >= int(np.load(f)["params"][8])]   # (short_hq: no matcher, the caller's case)


def rand_text(rng, n):
    return ACGT[rng.integers(0, 4, size=n)]


def resident(tm, dest, dest_is_src, rev_compl):
    """matchTexts as SimplePgMatcher calls it: leaves `dest` on the device -> the matches found"""
    return tm.matchTexts(pu.revcomp_np(dest) if rev_compl else dest, dest_is_src, rev_compl)


def raw(marks, n2, rev_compl):
    """(src, len, forward dst) rows -> matchTexts' coordinates"""
    m = np.asarray(marks, dtype=np.int64).reshape(-1, 3).copy()
    if rev_compl:
        m[:, 2] = n2 - (m[:, 2] + m[:, 1])
    return m.astype(np.uint64)


def check(tm, dest, matches, dest_is_src, rev_compl, min_len, src_len, pass_min=True, mapped_out=None):
    want = pu.mark_and_remove(dest, matches, dest_is_src, rev_compl, min_len, src_len)
    mapped, off, lens, info = tm.markAndRemoveExactMatches(matches, min_len if pass_min else None, mapped_out)
    assert lens.tobytes() == want[2], "lengths stream"
    assert off.tobytes() == want[1], "offsets stream"
    assert mapped.tobytes() == want[0], "mapped text"
    assert info["marks"] == want[0].count(b"%") and info["matched_symbols"] == dest.size - len(want[0]) + info["marks"]
    return mapped, off, lens, info


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("path", MAPPABLE, ids=lambda p: os.path.basename(p)[6:-4])
def test_reference_fixtures(path):
    z, texts, tl = load_case(path)
    hq = texts[0]
    tm = CopMEMMatcher(hq, tl, device=0)
    for p, dest in enumerate(texts):
        if not dest.size:
            continue
        found = resident(tm, dest, p == 0, True)
        for matches in (z[f"matches{p}"], found):
            mapped, off, lens, info = tm.markAndRemoveExactMatches(matches)
            assert mapped.tobytes() == z[f"mapped{p}"].tobytes(), (p, "mapped")
            assert off.tobytes() == z[f"off{p}"].tobytes() and lens.tobytes() == z[f"len{p}"].tobytes(), (p, "streams")
            assert info["marks"] == int((z[f"mapped{p}"] == pu.MATCH_MARK).sum())
    tm.close()


# ------------------------------------------------------------------------------------------------ round trip
@pytest.mark.parametrize("rev_compl", [True, False])
def test_round_trip_through_the_device_restore(rev_compl):
    hq, lq, nn = pu.make_texts(77, 300_000, 100_000, 30_000, nrep=150, chains=4, chain_depth=4)
    tl = 40
    tm = CopMEMMatcher(hq, tl, device=0)
    parts, total = [], 0
    for dest, dis in ((hq, True), (lq, False), (nn, False)):
        found = resident(tm, dest, dis, rev_compl)
        total += found.shape[0]
        mapped, off, lens, _ = check(tm, dest, found, dis, rev_compl, tl, hq.size, pass_min=False)
        parts.append((mapped.tobytes(), off.tobytes(), lens.tobytes()))
    tm.close()
    assert total > 100 and (nn == ord("N")).any()
    mapped, lens_m, offs, lns = pu.join_parts(parts)
    # (these texts hold no forward self-copy that overlaps its destination, which the device's restore would refuse)
    assert pu.hq_sources_valid(parts[0][0], parts[0][1], parts[0][2], hq.size)
    dec = PgRCDecoder(100, device=0)
    dec.restoreMatchedPgs(mapped, lens_m, hq.size, offs, lns, rev_compl)
    assert dec.text_lengths() == (hq.size, lq.size, nn.size)
    assert dec.text().tobytes() == hq.tobytes() + lq.tobytes() + nn.tobytes()
    dec.close()


# ------------------------------------------------------------------------------------------------ scan and block edges
@pytest.fixture(scope="module")
def mega():
    """a 1 Mbp destination against a 300 kbp source, resident as an LQ text matched on the reverse strand"""
    rng = np.random.default_rng(11)
    src, dest = rand_text(rng, 300_000), rand_text(rng, 1_000_003)
    tm = CopMEMMatcher(src, 40, device=0)
    resident(tm, dest, False, True)
    yield tm, src, dest, rng
    tm.close()


@pytest.mark.parametrize("unique", [0, 1, 2, 4095, 4096, 4097])
def test_unique_counts_at_the_scan_tile(mega, unique):
    tm, src, dest, rng = mega
    d = np.sort(rng.choice(dest.size // 100 - 1, unique, replace=False)) * 100 + rng.integers(0, 30, size=unique)
    ln = rng.integers(40, 70, size=unique)
    s = rng.integers(0, src.size - 70, size=unique)
    m = raw(np.stack([s, ln, d], axis=1), dest.size, True)
    if unique:
        m = np.concatenate([m, m[rng.integers(0, unique, size=unique // 3 + 1)]])[rng.permutation(unique + unique // 3 + 1)]   # duplicates
    info = check(tm, dest, m, False, True, 40, src.size)[3]
    assert info["unique_matches"] == unique and info["marks"] == unique


def test_pile_inside_a_long_match_then_a_chain_of_trimmed_ones(mega):
    tm, src, dest, rng = mega
    rows = [(0, 200_000, 1000)]
    for i in range(6000):                                   # start inside the long match; some reach past its end by >= min_len
        rows.append((int(rng.integers(0, 1000)), int(rng.integers(40, 400)), 1000 + int(rng.integers(1, 200_000))))
    at = 201_500
    for i in range(10_000):                                 # every one overlaps its predecessor: all trimmed, all kept
        rows.append((int(rng.integers(0, 1000)), 100, at))
        at += 60 - (i % 3)
    m = raw(rows, dest.size, True)
    info = check(tm, dest, m[rng.permutation(m.shape[0])], False, True, 40, src.size)[3]
    assert info["marks"] > 10_000


def test_more_matches_than_one_round_of_the_carry():
    """1 048 577 matches: more than 256 scan tiles of 4096, so the scan of the folds takes a second round"""
    rng = np.random.default_rng(12)
    n, n2 = 1_048_577, 64_000_000
    src, dest = rand_text(rng, 100_000), rand_text(rng, n2)
    tm = CopMEMMatcher(src, 40, device=0)
    resident(tm, dest, False, False)
    d = np.arange(n, dtype=np.int64) * 61 + rng.integers(0, 16, size=n)
    m = np.stack([rng.integers(0, src.size - 50, size=n), rng.integers(40, 46, size=n), d], axis=1).astype(np.uint64)
    info = check(tm, dest, m[rng.permutation(n)], False, False, 40, src.size)[3]
    assert info["marks"] == n and info["unique_matches"] == n
    tm.close()


# ------------------------------------------------------------------------------------------------ the text kernel's edges
def edge_marks(n2):
    """forward (src, len, dst): a mark at 0, literal runs of 1 .. 9 bytes, "%%", a mark that ends at n2"""
    rows, at = [(3, 40, 0)], 40
    for r in range(1, 10):
        at += r
        rows.append((10 + r, 40 + r, at))
        at += 40 + r
    at += 13
    rows += [(100, 44, at), (150, 41, at + 44)]             # adjacent
    rows.append((7, 45, n2 - 45))
    assert at + 85 < n2 - 45
    return rows


@pytest.mark.parametrize("n2", [16 * 64 + 1, 16 * 64 + 15])
@pytest.mark.parametrize("rev_compl", [True, False])
def test_text_kernel_edges_with_n(n2, rev_compl):
    rng = np.random.default_rng(n2)
    src, dest = rand_text(rng, 5000), rand_text(rng, n2).copy()
    rows = edge_marks(n2)
    for (_, ln, d), (_, _, d2) in zip(rows[:-1], rows[1:]):
        if d2 > d + ln:                                     # N at both edges of the literal run, i.e. next to both marks
            dest[d + ln] = dest[d2 - 1] = ord("N")
    dest[rows[-2][2] + rows[-2][1]] = ord("N")
    tm = CopMEMMatcher(src, 40, device=0)
    resident(tm, dest, False, rev_compl)
    mapped = check(tm, dest, raw(rows, n2, rev_compl), False, rev_compl, 40, src.size)[0].tobytes()
    assert mapped.startswith(b"%") and mapped.endswith(b"%") and b"%%" in mapped and b"%N%" in mapped and b"N%" in mapped
    # the same text without marks, and one with no N map at all
    check(tm, dest, np.zeros((0, 3), np.uint64), False, rev_compl, 40, src.size)
    plain = rand_text(rng, n2)
    resident(tm, plain, False, rev_compl)
    check(tm, plain, raw(rows, n2, rev_compl), False, rev_compl, 40, src.size)
    tm.close()


@pytest.mark.parametrize("rev_compl", [True, False])
def test_whole_text_as_one_match_and_the_destinations_own_buffer(rev_compl):
    rng = np.random.default_rng(5)
    src = rand_text(rng, 4000)
    tm = CopMEMMatcher(src, 40, device=0)
    lq = pu.revcomp_np(src[1000:1777]) if rev_compl else src[1000:1777].copy()
    resident(tm, lq, False, rev_compl)
    # (hand-made: the matcher itself, like the reference, leaves out a match's symbol at position 0 of the text it scans)
    whole = np.array([[1000, lq.size, 0]], np.uint64)
    mapped, off, lens, info = check(tm, lq, whole, False, rev_compl, 40, src.size)
    assert mapped.tobytes() == b"%" and info["marks"] == 1 and off.tobytes() == (1000).to_bytes(4, "little")
    # the source against itself, written over the caller's copy of it
    hq = src.copy()
    hq[3000:3300] = pu.revcomp_np(hq[100:400]) if rev_compl else hq[100:400]
    tm2 = CopMEMMatcher(hq, 40, device=0)
    found = resident(tm2, hq, True, rev_compl)
    assert found.shape[0] >= 1
    own = hq.copy()
    mapped = check(tm2, hq, found, True, rev_compl, 40, hq.size, mapped_out=own)[0]
    assert np.shares_memory(mapped, own) and b"%" in mapped.tobytes()
    tm.close()
    tm2.close()


# ------------------------------------------------------------------------------------------------ count, width, cap
def test_no_matches_and_the_target_length_default():
    rng = np.random.default_rng(6)
    src, dest = rand_text(rng, 3000), rand_text(rng, 2001)
    tm = CopMEMMatcher(src, 45, device=0)
    resident(tm, dest, False, True)
    mapped, off, lens, info = tm.markAndRemoveExactMatches(np.zeros((0, 3), np.uint64))     # min_match_len = UINT32_MAX
    assert mapped.tobytes() == dest.tobytes() and off.size == 0 and lens.tobytes() == bytes([45])
    assert info["marks"] == 0 and info["unique_matches"] == 0
    m = raw([(5, 44, 100), (9, 45, 300), (1, 300, 500)], dest.size, True)     # one below the target length
    assert check(tm, dest, m, False, True, 45, src.size, pass_min=False)[3]["marks"] == 2
    mapped, off, lens, _ = check(tm, dest, m, False, True, 200, src.size)         # min_len needs two bytes in the stream's head
    assert lens.tobytes()[:2] == bytes([128 + 200 % 128, 1])
    tm.close()


@pytest.mark.parametrize("nbytes,lo,hi", [(1, 0, 128), (2, 128, 16384), (3, 16384, 40000)])
def test_every_width_of_a_length_value(nbytes, lo, hi):
    rng = np.random.default_rng(nbytes)
    src, dest = rand_text(rng, 50_000), rand_text(rng, 400_007)
    tm = CopMEMMatcher(src, 40, device=0)
    resident(tm, dest, False, False)
    rows, at = [], 3
    for v in [lo, hi - 1] + rng.integers(lo, hi, size=6).tolist():
        rows.append((int(rng.integers(0, src.size - 40 - v)), 40 + v, at))
        at += 40 + v + int(rng.integers(0, 5))
    lens = check(tm, dest, raw(rows, dest.size, False), False, False, 40, src.size)[2]
    assert lens.size == 1 + nbytes * len(rows)
    tm.close()


def test_tiny_event_cap_still_leaves_the_destination(monkeypatch):
    monkeypatch.setenv("PGRC_MEM_EVENT_CAP", "7")
    hq, lq, _ = pu.make_texts(31, 60_000, 20_000, 0, nrep=40)
    tm = CopMEMMatcher(hq, 40, device=0)
    for dest, dis in ((lq, False), (hq, True)):
        found = resident(tm, dest, dis, True)
        assert found.shape[0] > 5
        check(tm, dest, found, dis, True, 40, hq.size)
    tm.close()


def test_eight_byte_offsets_above_4g_source_symbols():
    """a source of 2^32 + 3000 symbols (the generator of the full-size tests), an LQ text, a dozen hand-made marks whose sources
    lie above 2^32: 8-byte offsets, a 33-bit source field in the sort, bounds against a source length above UINT32_MAX.
    (29 s on an MI355X machine, nearly all of it making, uploading and indexing the 4.3 Gbp source: no smaller source has
    8-byte offsets.)"""
    from pgrc_amd import synth
    rng = np.random.default_rng(8)
    size = (1 << 32) + 3000
    src = synth.pg_host(synth.pg_params(size, seed=12345))
    dest = rand_text(rng, 60_001)
    tm = CopMEMMatcher(src, 45, device=0)
    resident(tm, dest, False, True)
    rows, at = [], 17
    for k in range(12):
        ln = int(rng.integers(45, 400))
        rows.append(((1 << 32) + int(rng.integers(0, 3000 - ln)) if k else size - ln, ln, at))
        at += ln + int(rng.integers(0, 3000))
    rows.append((77, 50, at))                                  # (and one below 2^32: the high word is zero, not garbage)
    m = raw(rows, dest.size, True)
    mapped, off, lens, info = check(tm, dest, m[rng.permutation(len(rows))], False, True, 45, size)
    assert off.size == 13 * 8 and info["marks"] == 13
    assert (np.frombuffer(off.tobytes(), "<u8")[:12] >= (1 << 32)).all()
    # a source that ends past the text's end is refused against the 64-bit length
    bad = m.copy()
    bad[0, 0] += np.uint64(1)
    with pytest.raises(PgrcMatchError) as e:
        tm.markAndRemoveExactMatches(bad, 45)
    assert e.value.code == E_PARAM
    tm.close()


def test_destination_shorter_than_k():
    """matchTexts of a text with no window at all still leaves it resident: mapped unchanged, and with a hand-made match"""
    rng = np.random.default_rng(10)
    src = rand_text(rng, 3000)
    tm = CopMEMMatcher(src, 40, device=0)
    for n2 in (1, 9, 17):
        for dis_rc in (True, False):
            dest = rand_text(rng, n2).copy()
            if n2 > 1:
                dest[n2 // 2] = ord("N")
            assert resident(tm, dest, False, dis_rc).shape[0] == 0
            mapped, off, lens, info = check(tm, dest, np.zeros((0, 3), np.uint64), False, dis_rc, 40, src.size)
            assert mapped.tobytes() == dest.tobytes() and off.size == 0 and lens.tobytes() == bytes([40])
            if n2 > 4:
                got = check(tm, dest, raw([(100, 4, 2)], n2, dis_rc), False, dis_rc, 3, src.size)[0].tobytes()
                assert got == dest[:2].tobytes() + b"%" + dest[6:].tobytes()
    tm.close()


# ------------------------------------------------------------------------------------------------ refused input
def test_refused_input_leaves_the_context_usable():
    rng = np.random.default_rng(9)
    src, dest = rand_text(rng, 3000), rand_text(rng, 2000)
    tm = CopMEMMatcher(src, 40, device=0)
    good = raw([(5, 50, 100), (9, 45, 300)], dest.size, True)

    def call(matches, min_len=40, cap=None, count=None):
        mt = np.ascontiguousarray(matches, dtype=np.uint64).reshape(-1, 3)
        buf = np.zeros(dest.size, np.uint8)
        mp = _lib.MemMapping()
        C.memset(C.byref(mp), 0x5A, C.sizeof(mp))
        rc = _lib.lib.pgrc_mem_mark_and_remove(tm._h, C.cast(mt.ctypes.data_as(C.c_void_p), C.POINTER(_lib.TextMatch)),
                                               mt.shape[0] if count is None else count, min_len, buf.ctypes.data_as(C.c_void_p),
                                               buf.size if cap is None else cap, C.byref(mp))
        return rc, mp

    def refused(code, *a, **kw):
        rc, mp = call(*a, **kw)
        assert rc == code and bytes(mp) == bytes(C.sizeof(mp))          # *out is cleared

    refused(E_STATE, good)                                              # no destination yet
    resident(tm, dest, False, True)
    bad = {"cap": (good, 40, dest.size - 1),
           "source end": (raw([(5, 50, 100), (src.size - 49, 50, 300)], dest.size, True),),
           "destination end": (np.array([[5, 50, dest.size - 49]], np.uint64),),
           "destination far off": (np.array([[5, 50, 2**63]], np.uint64),),
           "length 0": (raw([(5, 50, 100), (9, 0, 300)], dest.size, True),),
           "length 2^64-1": (np.array([[5, 2**64 - 1, 3]], np.uint64),),
           "min_len 0": (good, 0)}
    for what, args in bad.items():
        refused(E_PARAM, *args)
        rc, mp = call(good)                                             # the next valid call on the same context
        assert rc == 0 and mp.marks == 2, what
        _lib.lib.pgrc_mem_free_mapping(C.byref(mp))
        assert bytes(mp) == bytes(C.sizeof(mp))
    check(tm, dest, good, False, True, 40, src.size)
    # a failed matchTexts and a new source forget the destination
    with pytest.raises(PgrcMatchError):
        tm.matchTexts(dest, False, True, 5)                             # below K
    refused(E_STATE, good)
    resident(tm, dest, False, True)
    check(tm, dest, good, False, True, 40, src.size)
    tm._ck(_lib.lib.pgrc_mem_set_src_ascii(tm._h, tm._src.ctypes.data_as(C.c_void_p), tm._src.size))
    refused(E_STATE, good)
    tm.close()
