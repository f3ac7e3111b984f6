"""Pg-vs-Pg matching on texts that are already on the device (pgrc_mem_set_src_device, pgrc_mem_match_texts_device; DESIGN.md
4.21).  The packing kernel (mempack.hip) alone, through libpgrc_selftest.so, against tests/memdev_util.py's numpy reference --
which tests/test_memdev_reference.py holds to the host-reversed text on the CPU -- at every alignment, around its tile and in
the grid stride; then the two entry points against the host route on the host-reversed text and against the oracle: the
matches, the stale-register emulation without a host copy of either text, the mapping and the coded block that follow, the
chain from the assembler's text, and every refused call.  Device buffers are torch tensors; the library gets raw addresses."""
import functools

import numpy as np
import pytest
import torch

import memdev_util as mu
import oracle as orc
import pgasm_util as pa
import varlen_util as vu
from mem_util import COMBOS, make_pair, make_pg
from pgrc_amd import CopMEMMatcher, PgAssembler, PgrcMatchError, VarLenDNACoder

pytestmark = pytest.mark.gpu

E_PARAM, E_SYMBOL, E_STATE = 1, 5, 6
OFFSETS = (0, 1, 3, 7, 15)
T = mu.TILE_BYTES
LENGTHS = [1, 15, 16, 17, 31, 32, 33, 45, 255, 256, 257, T - 1, T, T + 1, 2 * T + 5]


def dev(text, off=0):
    """a copy of the text `off` bytes into a 16-byte-aligned device allocation, bytes outside ACGNT in front of it and behind it
    (a kernel that packed one of them would raise the flag) -> (the tensor, to be kept alive; the text's device address)"""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    buf = np.full(off + text.size + 48, ord("%"), dtype=np.uint8)
    buf[off:off + text.size] = text
    t = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + off


@pytest.fixture(scope="module")
def mp():
    h = mu.MemPack(0)
    yield h
    h.close()


# ---------------------------------------------------------------------------------------------- 1. the packing kernel
def variants(n, seed):
    """(name, text): without N; with N at the first and the last byte and across a word boundary; with one byte outside ACGNT"""
    rng = np.random.default_rng(seed)
    bad = mu.random_text(n, seed + 2, bad_at=int(rng.integers(0, n)))
    return [("clean", mu.random_text(n, seed)), ("n", mu.random_text(n, seed + 1, n_at=(0, n - 1, 15, 16, n // 2))), ("bad", bad)]


def check_packing(mp, n, block_cap=0):
    for name, text in variants(n, 11 * n):
        want = {rev: mu.pack_ref(text, rev) for rev in (False, True)}
        for off in OFFSETS:
            keep, ptr = dev(text, off)
            for rev in (False, True):
                words, nmap, flags, guards = mp.pack(ptr, n, rev, block_cap)
                what = f"n {n}, {name}, offset {off}, {'reversed' if rev else 'forward'}"
                ww, wn, wf = want[rev]
                assert guards == 7, f"{what}: guard zones written (bit 0 words, 1 N map, 2 flag): {guards:#x}"
                assert flags == wf, f"{what}: flags {flags}, expected {wf}"
                if name == "bad":
                    continue                                # (the flag only: the words of a refused text mean nothing)
                assert np.array_equal(words, ww), f"{what}: words differ at {np.flatnonzero(words != ww)[:8]} of {ww.size} (pad included)"
                assert np.array_equal(nmap, wn), f"{what}: N map differs at {np.flatnonzero(nmap != wn)[:8]}"
            del keep
    # the source's form: no N map is written at all, an N raises bit 1 as it does with one
    name, text = variants(n, 11 * n)[1]
    keep, ptr = dev(text, 3)
    words, nmap, flags, guards = mp.pack(ptr, n, False, block_cap, with_nmap=False)
    assert guards == 7 and flags == 2 and np.array_equal(words, mu.pack_ref(text, False)[0])
    assert np.array_equal(nmap, np.full(nmap.size, 0xA5A5, dtype=np.uint16)), "an N map was written without being asked for"


@pytest.mark.parametrize("n", LENGTHS)
def test_packing_kernel_equals_numpy_at_every_alignment(mp, n):
    check_packing(mp, n)


def test_packing_kernel_in_the_grid_stride(mp):
    """100 003 bytes = 25 tiles in two blocks: every block packs a dozen tiles, one after the other"""
    check_packing(mp, 100_003, block_cap=2)


# ---------------------------------------------------------------------------------------------- 2. the matches
@functools.lru_cache(maxsize=2)
def pair(seed, with_n, low_complexity):
    return make_pair(seed, with_n=with_n, low_complexity=low_complexity)


def four_routes(src, other, combos=COMBOS, target_len=45, what=""):
    """every combination of a host / device source with a host / device destination against the oracle -> matches found"""
    keep_s, ps = dev(src, 0)
    keep_o, po = dev(other, 5)
    host, resident = CopMEMMatcher(src, target_len, device=0), CopMEMMatcher(None, target_len, device=0)
    resident.setSrcDevice(ps, src.size)
    total = 0
    for dest_is_src, rev_compl in combos:
        d = orc.mem_dest(src, other, dest_is_src, rev_compl)
        o = orc.oracle_mem_match(src, d, dest_is_src, rev_compl, target_len)
        ptr, n2 = (ps, src.size) if dest_is_src else (po, other.size)
        got = {"host source, host destination": host.matchTexts(d, dest_is_src, rev_compl),
               "device source, device destination": resident.matchTextsDevice(ptr, n2, dest_is_src, rev_compl),
               "device source, host destination": resident.matchTexts(d, dest_is_src, rev_compl),
               "host source, device destination": host.matchTextsDevice(ptr, n2, dest_is_src, rev_compl)}
        if dest_is_src:
            got["device source, no destination pointer"] = resident.matchTextsDevice(0, n2, True, rev_compl)
        for route, g in got.items():
            assert np.array_equal(g, o), f"{what} {route}: destIsSrc={dest_is_src} rc={rev_compl}: {len(g)} / {len(o)} matches"
        total += len(o)
    host.close()
    resident.close()
    return total


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("with_n,low_complexity", [(False, False), (True, False), (False, True), (True, True)])
def test_device_route_finds_the_matches_of_the_host_route_and_the_oracle(seed, with_n, low_complexity):
    src, other = pair(seed, with_n, low_complexity)
    assert four_routes(src, other, what=f"seed {seed}") > 100


# ---------------------------------------------------------------------------------------------- 3. ragged lengths
def test_device_route_short_and_ragged_texts():
    src, other = make_pair(3, G=30000, G2=2000)
    keep_s, ps = dev(src, 9)
    keep_o, po = dev(other, 2)
    m = CopMEMMatcher(None, 45, device=0)
    m.setSrcDevice(ps, src.size)
    for n2 in (1, 31, 32, 33, 45, 100, 400, 767, 768, 769, 770, 800, 1535, 1536, 1537, 2000):
        d = orc.mem_dest(src, other[:n2], 0, 1)
        g = m.matchTextsDevice(po, n2, False, True)
        assert np.array_equal(g, orc.oracle_mem_match(src, d, 0, 1)), n2
    m.close()


# ---------------------------------------------------------------------------------------------- 4. stale registers
def test_device_route_stale_registers_without_a_host_copy():
    """The construction of test_gpu_mem.py's test_mem_matches_touching_the_text_ends_and_stale_registers: source K-mers at the
    very start / end of the source copied all over the destination.  Neither text has a host copy here, so the 4-byte looks
    of the register emulation are rebuilt from the packed words on the device."""
    rng = np.random.default_rng(5)
    src = make_pg(120000, 55, nrep=50)
    other = make_pg(40000, 56, nrep=5)
    head, tail = src[:70].copy(), src[-70:].copy()
    for k in range(40):
        seg = (head, tail)[k % 2][: int(rng.integers(46, 70))] if k % 4 < 2 else (head, tail)[k % 2][-int(rng.integers(46, 70)):]
        d = int(rng.integers(100, other.size - 100))
        other[d:d + seg.size] = orc.revcomp_ascii(seg) if k % 3 else seg
    other[:60] = orc.revcomp_ascii(src[-60:])
    other[-60:] = orc.revcomp_ascii(src[:60])
    keep_s, ps = dev(src, 1)
    keep_o, po = dev(other, 7)
    m = CopMEMMatcher(None, 45, device=0)
    m.setSrcDevice(ps, src.size)
    host = CopMEMMatcher(src, 45, device=0)
    stale = stale_host = 0
    for dest_is_src, rev_compl in COMBOS:
        d = orc.mem_dest(src, other, dest_is_src, rev_compl)
        ptr, n2 = (ps, src.size) if dest_is_src else (po, other.size)
        g = m.matchTextsDevice(ptr, n2, dest_is_src, rev_compl)
        stale += m.counters()["stale_lookups"]
        assert np.array_equal(g, orc.oracle_mem_match(src, d, dest_is_src, rev_compl)), (dest_is_src, rev_compl)
        host.matchTexts(d, dest_is_src, rev_compl)
        stale_host += host.counters()["stale_lookups"]
    assert stale > 0 and stale == stale_host        # the counter means what it means on the host route
    m.close()
    host.close()


# ---------------------------------------------------------------------------------------------- 5. downstream
def encoder_book():
    for _, _, streams in vu.load_fixtures():
        if 0 in streams:
            return vu.parse_stream(streams[0])[2]
    raise KeyError("no fixture coded with book 0")


def test_mapping_and_coded_block_after_the_device_route():
    """markAndRemoveExactMatches, and the resident mapping + encodeMapped, after matchTextsDevice give the bytes they give after
    matchTexts on the host-reversed text: HQ against itself, LQ and an N text against HQ, as matchPgsInPg runs them"""
    hq, lq = make_pair(4, G=120000, G2=40000)
    _, ntext = make_pair(6, G=120000, G2=3000, with_n=True)
    ntext[200:500] = orc.revcomp_ascii(hq[7000:7300])
    ntext[300] = ord("N")
    texts = [hq, lq, ntext]
    keep = [dev(t, off) for t, off in zip(texts, (0, 3, 11))]
    host, resident = CopMEMMatcher(hq, 45, device=0), CopMEMMatcher(None, 45, device=0)
    resident.setSrcDevice(keep[0][1], hq.size)
    book = encoder_book()
    coder = VarLenDNACoder(book.raw + b"\0", device=0)
    mapped = {}
    for p in (1, 2, 0):
        found = host.matchTexts(orc.revcomp_ascii(texts[p]), p == 0, True)
        found_d = resident.matchTextsDevice(keep[p][1], texts[p].size, p == 0, True)
        assert np.array_equal(found, found_d) and (p == 2 or len(found) > 10), p
        a, b = host.markAndRemoveExactMatches(found), resident.markAndRemoveExactMatches(found_d)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3], p
        assert p != 2 or (ord("N") in a[0] and ord("%") in a[0])
        mapped[p] = a[0].copy()
        ra, rb = host.markAndRemoveExactMatchesResident(found, p), resident.markAndRemoveExactMatchesResident(found_d, p)
        assert ra[0] == rb[0] == a[0].size and ra[1].tobytes() == rb[1].tobytes() == a[1].tobytes() and ra[2].tobytes() == rb[2].tobytes(), p
    ca, la = host.encodeMapped(coder)
    cb, lb = resident.encodeMapped(coder)
    assert la == lb == tuple(mapped[p].size for p in range(3))
    assert ca.tobytes() == cb.tobytes() == vu.encode_serial(book, np.concatenate([mapped[0], mapped[1], mapped[2]]))
    host.close()
    resident.close()
    coder.close()


# ---------------------------------------------------------------------------------------------- 6. the chain
def test_assembled_texts_go_straight_into_the_matcher():
    """PgAssembler.text_device() -> setSrcDevice / matchTextsDevice, with 4 symbols (the source) and with 5 (a destination with
    N's that shares its first chain's text with the source); the assembler runs again before the matching, so a borrowed
    source would be gone"""
    shape = dict(L=60, chains=[1500, 900, 400], cycles=[40], singles=30, mean_shift=12)
    c4 = pa.make_case(seed=41, symbols=4, **shape)
    c5 = pa.make_case(seed=41, symbols=5, n_share=0.004, **shape)
    asm = PgAssembler(device=0)
    asm.run(c4["rows"], c4["next_read"], c4["overlap"], 60, 4)
    src = asm.text().copy()
    p, n = asm.text_device()
    assert n == src.size and n > 20000
    resident = CopMEMMatcher(None, 45, device=0)
    resident.setSrcDevice(p, n)
    asm.run(c5["rows"], c5["next_read"], c5["overlap"], 60, 5)        # (the assembler's text buffer now holds another text)
    other = asm.text().copy()
    p2, n2 = asm.text_device()
    assert n2 == other.size and ord("N") in other
    host = CopMEMMatcher(src, 45, device=0)
    total = 0
    for dest_is_src, rev_compl in COMBOS:
        d = orc.mem_dest(src, other, dest_is_src, rev_compl)
        want = host.matchTexts(d, dest_is_src, rev_compl)
        got = resident.matchTextsDevice(0 if dest_is_src else p2, src.size if dest_is_src else n2, dest_is_src, rev_compl)
        assert np.array_equal(got, want) and np.array_equal(got, orc.oracle_mem_match(src, d, dest_is_src, rev_compl)), (dest_is_src, rev_compl)
        total += len(got)
        a, b = host.markAndRemoveExactMatches(want), resident.markAndRemoveExactMatches(got)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])), (dest_is_src, rev_compl)
    assert total > 10
    for h in (asm, resident, host):
        h.close()


# ---------------------------------------------------------------------------------------------- 7. errors
def test_refused_calls_leave_the_context_usable():
    src, other = make_pair(1, G=20000, G2=3000)
    keep_s, ps = dev(src, 5)
    keep_o, po = dev(other, 0)
    want = orc.oracle_mem_match(src, orc.mem_dest(src, other, 0, 1), 0, 1)
    assert len(want) > 0

    def usable(m):
        assert np.array_equal(m.matchTextsDevice(po, other.size, False, True), want)

    def refused(code, call, *args):
        with pytest.raises(PgrcMatchError) as e:
            call(*args)
        assert e.value.code == code, (e.value.code, str(e.value))

    m = CopMEMMatcher(None, 45, device=0)
    refused(E_STATE, m.matchTextsDevice, po, other.size, False, True)                  # no source yet
    pinned = torch.from_numpy(src.copy()).pin_memory()
    refused(E_PARAM, m.setSrcDevice, src.ctypes.data, src.size)                        # pageable host memory
    refused(E_PARAM, m.setSrcDevice, pinned.data_ptr(), src.size)                      # page-locked host memory
    refused(E_STATE, m.matchTextsDevice, po, other.size, False, True)                  # (still none)
    bad = src.copy()
    bad[777] = ord("N")                                                                # the source must be over ACGT
    keep_b, pb = dev(bad, 2)
    refused(E_SYMBOL, m.setSrcDevice, pb, bad.size)
    assert "outside ACGT" in (m_err := last_error(m)), m_err
    refused(E_STATE, m.matchTextsDevice, po, other.size, False, True)
    m.setSrcDevice(ps, src.size)
    usable(m)
    refused(E_PARAM, m.matchTextsDevice, other.ctypes.data, other.size, False, True)   # a host destination through the device form
    refused(E_PARAM, m.matchTextsDevice, pinned.data_ptr(), src.size, True, True)      # ... even where it would not be read
    usable(m)
    bad2 = other.copy()
    bad2[100] = ord("%")
    keep_b2, pb2 = dev(bad2, 1)
    refused(E_SYMBOL, m.matchTextsDevice, pb2, bad2.size, False, True)
    refused(E_STATE, m.markAndRemoveExactMatches, want)                                # a failed call leaves nothing to map
    usable(m)
    assert len(m.matchTextsDevice(pb2 + 95, 10, False, True)) == 0                     # shorter than K: accepted as on the host route ...
    refused(E_STATE, m.markAndRemoveExactMatches, np.zeros((0, 3), np.uint64))         # ... but not remembered
    assert len(m.matchTextsDevice(po, 10, False, True)) == 0                           # a clean short text is
    assert m.markAndRemoveExactMatches(np.zeros((0, 3), np.uint64))[0].tobytes() == other[:10].tobytes()
    refused(E_PARAM, m.matchTextsDevice, po, other.size, True, True)                   # dest_is_src with another length
    refused(E_PARAM, m.matchTextsDevice, po, other.size, False, False, 20)             # minMatchLength < K (:606-609)
    refused(E_PARAM, m.matchTextsDevice, 0, other.size, False, True)                   # no pointer without dest_is_src
    usable(m)
    m.close()


def last_error(m):
    from pgrc_amd import _lib
    return (_lib.lib.pgrc_mem_last_error(m._h) or b"").decode()
