"""The variable-length DNA coder on the device (pgrc_varlen_encode / _decode, varlen.hip) and the two stages around it
(pgrc_mem_mark_and_remove_resident + pgrc_mem_encode_mapped, pgrc_decode_set_mapped_text_coded): byte for byte against what the
reference wrote (tests/golden/varlen_*.npz) with the book of each of its three ids, host to host and device to device; at the
edges of the kernels (the thread's run, the block's tile, the scan's tile, the 16 alignments of the source and of the output)
against tests/varlen_util.encode_serial; over three parts cut everywhere; over every refused input; above 2^32 symbols without a
host copy; and through matchTexts -> the resident mapping -> the coder -> the coded restore, back to the original texts."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pgmap_util as pu
import varlen_util as vu
from pgrc_amd import CopMEMMatcher, PgRCDecoder, PgrcMatchError, VarLenDNACoder, _lib
from test_pgmap_oracle import load_case

pytestmark = pytest.mark.gpu
E_PARAM, E_SYMBOL, E_STATE = 1, 5, 6
K = vu.source_constants()
RUN, TILE, DRUN, DTILE, EPB = K["VL_RUN"], K["VL_TILE"], K["VL_DRUN"], K["VL_DTILE"], K["SCO_EPB"]
FIXTURES = vu.load_fixtures()
CASES = [(name, text, bid, stream) for name, text, streams in FIXTURES for bid, stream in sorted(streams.items())]
ACGT = np.frombuffer(b"ACGT", np.uint8)
ALPHABET = np.frombuffer(b"ACGTN%", np.uint8)


def book_of(bid) -> vu.Book:
    for _, _, streams in FIXTURES:
        if bid in streams:
            return vu.parse_stream(streams[bid])[2]
    raise KeyError(bid)


@pytest.fixture(scope="module")
def coders():
    made = {bid: (VarLenDNACoder(book_of(bid).raw + b"\0", device=0), book_of(bid)) for bid in vu.BOOK_IDS}
    yield made
    for c, _ in made.values():
        c.close()


def dev(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8).copy()).cuda()


def host(t) -> bytes:
    return t.cpu().numpy().tobytes() if isinstance(t, torch.Tensor) else np.asarray(t).tobytes()


def decode_np(book: vu.Book, coded: np.ndarray) -> np.ndarray:
    """vu.decode for long streams"""
    tab = np.zeros((256, 4), np.uint8)
    lens = np.zeros(256, np.int64)
    for i, c in enumerate(book.codes):
        tab[i, :len(c)] = list(c)
        lens[i] = len(c)
    rows = tab[coded]
    return rows[np.arange(4)[None, :] < lens[coded][:, None]]


def check_parse(book: vu.Book, text: np.ndarray, coded: np.ndarray) -> None:
    """`coded` is the reference's parse of `text`: it starts at 0, and at every position it visits the code and the step are
    the ones the look-up rule gives there (so, position by position, it is the serial loop's output); vectorised"""
    lens = np.array([len(c) for c in book.codes] + [0] * (256 - len(book.codes)), np.int64)[coded]
    pos = np.concatenate([[0], np.cumsum(lens)])
    n = text.size
    assert pos[-1] == n, "the codes do not cover the text"
    pos = pos[:-1]
    pad = np.concatenate([text, np.zeros(4, np.uint8)])
    t = (pad[pos].astype(np.uint32) | pad[pos + 1].astype(np.uint32) << 8 | pad[pos + 2].astype(np.uint32) << 16
         | (pad[pos + 3].astype(np.uint32) & 7) << 24)
    keys = np.array(sorted(book.lut), dtype=np.uint32)
    vals = np.array([book.lut[int(k)] for k in keys], dtype=np.uint8)

    def look(q):
        at = np.minimum(np.searchsorted(keys, q), keys.size - 1)
        return np.where(keys[at] == q, vals[at], 0).astype(np.uint8)

    rem = n - pos
    f4, f3, f2, f1 = np.where(rem >= 4, look(t), 0), np.where(rem >= 3, look(t & 0xFFFFFF), 0), np.where(rem >= 2, look(t & 0xFFFF), 0), look(t & 0xFF)
    want = np.where(f4 > 0, f4, np.where(f3 > 0, f3, np.where(f2 > 0, f2, f1)))
    step = np.where(f4 > 0, 4, np.where(f3 > 0, 3, np.where(f2 > 0, 2, 1)))
    assert np.array_equal(want, coded) and np.array_equal(step, lens)


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name,text,bid,stream", CASES, ids=[f"{c[0]}-{c[2]}" for c in CASES])
def test_reference_fixtures(coders, name, text, bid, stream):
    coder, _ = coders[bid]
    _, _, book, payload = vu.parse_stream(stream)
    assert book.raw == coders[bid][1].raw
    got = coder.encode(text)                                            # host to host
    assert isinstance(got, np.ndarray) and got.tobytes() == payload
    assert coder.decode(payload, text.size).tobytes() == text.tobytes()
    d_text = dev(text)                                                  # device to device
    d_coded = coder.encode(d_text)
    assert d_coded.is_cuda and host(d_coded) == payload
    d_back = coder.decode(d_coded, text.size)
    assert d_back.is_cuda and torch.equal(d_back, d_text)
    assert coder.decode(dev(np.frombuffer(payload, np.uint8)), text.size, out=np.empty(text.size, np.uint8)).tobytes() == text.tobytes()
    tm = coder.timing()
    assert tm["was_decode"] == 1 and tm["symbols"] == text.size and tm["coded_bytes"] == len(payload)


# ------------------------------------------------------------------------------------------------ the kernels' edges
def edge_lengths():
    ns = set(range(0, 10))
    for base in (RUN, 2 * RUN, TILE, 2 * TILE):
        ns |= {base + d for d in range(-4, 5)}
    ns |= {3 * TILE + 5, TILE - RUN, TILE + RUN + 1}
    return sorted(ns)


@pytest.mark.parametrize("bid", vu.BOOK_IDS)
def test_every_length_at_the_run_and_the_tile(coders, bid):
    coder, book = coders[bid]
    rng = np.random.default_rng(100 + bid)
    big = ALPHABET[rng.choice(6, size=3 * TILE + 5, p=[.24, .24, .24, .24, .02, .02])]
    d_big = dev(big)
    for n in edge_lengths():
        want = vu.encode_serial(book, big[:n])
        assert coder.encode(big[:n]).tobytes() == want, n
        got = coder.encode(d_big[:n])
        assert host(got) == want, n
        assert host(coder.decode(got, n)) == big[:n].tobytes(), n
    assert coder.decode(b"", 0).size == 0


def test_the_scan_tile_of_blocks(coders):
    """SCO_EPB blocks and a few symbols: the scan of the blocks' maps and of their counts takes a second block of its own, and
    the carry between them is a fold of folds.  The longest text is checked position by position (check_parse); the others
    share its parse up to a position near their end and are finished by the serial loop from there."""
    coder, book = coders[0]
    rng = np.random.default_rng(7)
    n_max = EPB * TILE + 4
    text = ACGT[rng.integers(0, 4, size=n_max)].copy()
    text[rng.random(n_max) < 1 / 500] = ord("%")
    d_text = dev(text)
    out = torch.empty(n_max // 2, dtype=torch.uint8, device="cuda")
    full = coder.encode(d_text, out=out).cpu().numpy().copy()
    check_parse(book, text, full)
    lens = np.array([len(c) for c in book.codes], np.int64)[full]
    pos = np.concatenate([[0], np.cumsum(lens)])
    for n in range(EPB * TILE - 4, n_max):
        k = int(np.searchsorted(pos, n - 8, side="right")) - 1          # the last position of the parse at or before n - 8
        want = full[:k].tobytes() + vu.encode_serial(book, text[pos[k]:n])
        assert host(coder.encode(d_text[:n], out=out)) == want, n
    # the decoder's scan tile: SCO_EPB blocks of codes, every byte value (codes the book leaves empty or does not have)
    m = EPB * DTILE + 3
    coded = rng.integers(0, 256, size=m).astype(np.uint8)
    want = decode_np(book, coded)
    got = coder.decode(dev(coded), want.size)
    assert torch.equal(got.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("bid", vu.BOOK_IDS)
def test_decode_lengths_at_the_run_and_the_tile(coders, bid):
    coder, book = coders[bid]
    rng = np.random.default_rng(200 + bid)
    coded = rng.integers(0, 256, size=3 * DTILE + 5).astype(np.uint8)
    d_coded = dev(coded)
    ms = set(range(0, 10)) | {b + d for b in (DRUN, DTILE, 2 * DTILE) for d in range(-2, 3)} | {3 * DTILE + 5}
    for m in sorted(ms):
        want = vu.decode(book, coded[:m].tobytes())
        assert coder.decode(coded[:m], len(want)).tobytes() == want, m
        assert host(coder.decode(d_coded[:m], len(want))) == want, m
        if m > 16:                                                       # a coded stream that starts at every alignment
            off = m % 16
            assert host(coder.decode(d_coded[off:m], len(vu.decode(book, coded[off:m].tobytes())))) == vu.decode(book, coded[off:m].tobytes())


def test_one_symbol_across_blocks_entries_never_merge(coders):
    for bid in vu.BOOK_IDS:
        coder, book = coders[bid]
        for sym in b"A%N":
            for n in (4 * TILE + 3, 4 * TILE + 1):
                text = np.full(n, sym, np.uint8)
                want = vu.encode_serial(book, text)
                assert host(coder.encode(dev(text))) == want, (bid, chr(sym), n)


def test_a_mark_at_each_place_of_a_window_at_the_edges(coders):
    coder, book = coders[0]
    rng = np.random.default_rng(9)
    base = ACGT[rng.integers(0, 4, size=2 * TILE + 100)]
    d_text = dev(base)
    for edge in (RUN, TILE, 2 * TILE):
        for d in range(-4, 4):                                           # the four places of the windows that straddle the edge
            text = base.copy()
            text[edge + d] = ord("%")
            d_text[edge + d] = ord("%")
            assert host(coder.encode(d_text)) == vu.encode_serial(book, text), (edge, d)
            d_text[edge + d] = int(base[edge + d])


def test_every_alignment_of_the_source_and_of_the_output(coders):
    coder, book = coders[0]
    rng = np.random.default_rng(10)
    n = 2 * TILE + 77
    text = ALPHABET[rng.choice(6, size=n, p=[.24, .24, .24, .24, .02, .02])]
    want = vu.encode_serial(book, text)
    room = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(len(want) + 64, dtype=torch.uint8, device="cuda")
    for off in range(16):
        room[off:off + n] = torch.from_numpy(text)
        out.fill_(0xEE)
        got = coder.encode(room[off:off + n], out=out[15 - off:15 - off + len(want)])
        assert host(got) == want, off
        assert bool((out[:15 - off] == 0xEE).all()) and bool((out[15 - off + len(want):] == 0xEE).all()), off   # nothing outside
        back = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        coder.decode(got, n, out=back[off:off + n])
        assert host(back[off:off + n]) == text.tobytes() and bool((back[:off] == 0xEE).all()) and bool((back[off + n:] == 0xEE).all()), off


# ------------------------------------------------------------------------------------------------ parts
def test_three_parts_cut_everywhere(coders):
    coder, book = coders[0]
    rng = np.random.default_rng(11)
    text = ALPHABET[rng.choice(6, size=TILE + 333, p=[.24, .24, .24, .24, .02, .02])]
    want = vu.encode_serial(book, text)
    cuts = [(a, a + w) for a in range(40, 44) for w in (0, 1, 2, 3, 5, 61, 62, 63, 64)]          # every residue mod 4, parts of 0 .. 3
    cuts += [(0, 0), (0, 1), (1, 3), (text.size - 2, text.size - 1), (text.size, text.size), (TILE - 1, TILE + 1), (RUN - 1, RUN + 2)]
    for i, (a, b) in enumerate(cuts):
        parts = [text[:a], text[a:b], text[b:]]
        mixed = [dev(p) if (i >> k) & 1 else p for k, p in enumerate(parts)]                     # host and device parts mixed
        assert coder.encode(mixed, out=np.empty(text.size, np.uint8)).tobytes() == want, (a, b)
    # a window that spans all three: parts of one and two symbols in the middle of a text of seven
    small = text[:7]
    for a, b in ((1, 2), (1, 3), (2, 3), (3, 4)):
        got = coder.encode([dev(small[:a]), small[a:b], dev(small[b:])], out=np.empty(7, np.uint8))
        assert got.tobytes() == vu.encode_serial(book, small), (a, b)
    assert coder.encode([text[:100], text[100:]]).tobytes() == want[:0] + vu.encode_serial(book, text)   # two parts
    assert coder.encode([]).size == 0 and coder.encode([b"", b"", b""]).size == 0


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_input_leaves_the_coder_usable(coders):
    coder, book = coders[0]
    rng = np.random.default_rng(12)
    text = ACGT[rng.integers(0, 4, size=TILE + 50)]
    want = vu.encode_serial(book, text)

    def fails(code, fn):
        with pytest.raises(PgrcMatchError) as e:
            fn()
        assert e.value.code == code
        assert coder.encode(text).tobytes() == want                     # the coder is still usable

    for at in (0, RUN, TILE - 1, text.size - 1):                        # a byte outside the book, also as the last one
        for byte in (ord("X"), ord("a"), 0, ord("I")):                  # ('I' shares its low three bits with 'A')
            bad = text.copy()
            bad[at] = byte
            fails(E_SYMBOL, lambda: coder.encode(bad))
    bad = text.copy()
    bad[-1] = ord("X")
    fails(E_SYMBOL, lambda: coder.encode([dev(text[:10]), text[10:20], dev(bad[20:])]))          # in the last part
    fails(E_SYMBOL, lambda: coder.encode([text[:10], np.frombuffer(b"R", np.uint8), text[10:]]))
    out = np.full(len(want) - 1, 0xEE, np.uint8)
    fails(E_PARAM, lambda: coder.encode(text, out=out))                 # capacity one short
    assert (out == 0xEE).all()
    n = C.c_uint64(0)
    part = _lib.VarLenPart(text.ctypes.data, text.size, 0)
    assert _lib.lib.pgrc_varlen_encode(coder._h, C.byref(part), 1, out.ctypes.data, out.size, 0, C.byref(n)) == E_PARAM and n.value == len(want)
    assert _lib.lib.pgrc_varlen_encode(coder._h, C.byref(part), 4, out.ctypes.data, out.size, 0, C.byref(n)) == E_PARAM
    part_dev = _lib.VarLenPart(text.ctypes.data, text.size, 1)          # a host pointer flagged as a device pointer
    assert _lib.lib.pgrc_varlen_encode(coder._h, C.byref(part_dev), 1, out.ctypes.data, out.size, 0, C.byref(n)) == E_PARAM
    for delta in (-1, 1):                                               # decode with an expected length one off
        fails(E_PARAM, lambda: coder.decode(want, text.size + delta, out=np.empty(text.size + 1, np.uint8)))
    d_out = torch.full((text.size + 1,), 0xEE, dtype=torch.uint8, device="cuda")
    fails(E_PARAM, lambda: coder.decode(dev(np.frombuffer(want, np.uint8)), text.size + 1, out=d_out))
    assert bool((d_out == 0xEE).all())                                  # nothing written
    assert coder.decode(want, text.size).tobytes() == text.tobytes()


@pytest.mark.parametrize("what,book", [
    ("257 codes", b"\n".join([b"A", b"C", b"G", b"T"] + [b""] * 253)),
    ("a 5-byte code", b"A\nC\nG\nT\nACGTA"),
    ("a two-symbol code 0", b"AC\nA\nC"),
    ("a symbol without a one-symbol code", b"A\nC\nAG"),
    ("two symbols sharing their low three bits", b"A\nC\nG\nT\nI"),
    ("a symbol whose low three bits are 0", b"A\nC\nG\nT\nH"),            # 'H' 0x48
])
def test_refused_books(coders, what, book):
    with pytest.raises(PgrcMatchError) as e:
        VarLenDNACoder(book, device=0)
    assert e.value.code == E_PARAM, what
    coder, ref = coders[0]
    assert coder.encode(b"ACGTACGTA").tobytes() == vu.encode_serial(ref, np.frombuffer(b"ACGTACGTA", np.uint8))


def test_a_small_book_of_ones_own(coders):
    """a book that is not one of the reference's three: fewer than 256 codes, no trailing NUL, a code that overwrites an
    earlier one's key, a four-symbol code whose last symbol only counts by its low three bits"""
    raw = b"A\nC\nG\nT\nACGT\nAC\nGT\n\nAC\nTTT"
    book = vu.Book(raw)
    coder = VarLenDNACoder(raw, device=0)
    rng = np.random.default_rng(13)
    for n in (1, 2, 3, 4, 5, 100, TILE + 7):
        text = ACGT[rng.integers(0, 4, size=n)]
        want = vu.encode_serial(book, text)
        assert coder.encode(text).tobytes() == want
        assert coder.decode(want, n).tobytes() == text.tobytes()
    assert coder.decode(bytes([0, 200, 255, 7, 9]), 4).tobytes() == b"ATTT"     # codes the book does not have decode to nothing
    coder.close()


# ------------------------------------------------------------------------------------------------ above 2^32
def test_above_4g_symbols_without_a_host_copy(coders):
    coder, book = coders[0]
    n = (1 << 32) + 4099
    text = torch.full((n,), ord("A"), dtype=torch.uint8, device="cuda")
    out = torch.empty(n // 4 + 16, dtype=torch.uint8, device="cuda")
    coded = coder.encode(text, out=out)
    aaaa, aaa = book.lut[int.from_bytes(b"AAAA", "little") & vu.LUT_MASK], book.lut[int.from_bytes(b"AAA\0", "little")]
    assert coded.numel() == n // 4 + 1 and n % 4 == 3
    assert bool(torch.all(coded[:-1] == aaaa)) and int(coded[-1]) == aaa
    text.fill_(0)
    back = coder.decode(coded, n, out=text)
    assert back.numel() == n and bool(torch.all(back == ord("A")))
    with pytest.raises(PgrcMatchError) as e:
        coder.decode(coded, n - 1, out=text)
    assert e.value.code == E_PARAM


# ------------------------------------------------------------------------------------------------ through the stages
MAPPABLE = [(name, streams[0]) for name, _, streams in FIXTURES
            if name.startswith("pgmap_") and int(np.load(os.path.join(vu.GOLDEN, name + ".npz"))["params"][1]) >= int(np.load(os.path.join(vu.GOLDEN, name + ".npz"))["params"][8])]


@pytest.mark.parametrize("name,stream", MAPPABLE, ids=[m[0][6:] for m in MAPPABLE])
def test_match_map_code_and_restore(coders, name, stream):
    coder, _ = coders[0]
    z, texts, tl = load_case(os.path.join(vu.GOLDEN, name + ".npz"))
    hq = texts[0]
    payload = vu.parse_stream(stream)[3]
    tm = CopMEMMatcher(hq, tl, device=0)
    with pytest.raises(PgrcMatchError) as e:
        tm.encodeMapped(coder)
    assert e.value.code == E_STATE                                      # no resident HQ or LQ yet
    streams = {}
    for p in (1, 2, 0):                                                 # LQ, N, then HQ against itself, as matchPgsInPg does
        dest = texts[p]
        if not dest.size:
            continue
        found = tm.matchTexts(pu.revcomp_np(dest), p == 0, True)
        mapped_len, off, lens, info = tm.markAndRemoveExactMatchesResident(found, p)
        assert mapped_len == z[f"mapped{p}"].size and off.tobytes() == z[f"off{p}"].tobytes() and lens.tobytes() == z[f"len{p}"].tobytes()
        streams[p] = (off, lens)
    coded, lens3 = tm.encodeMapped(coder)
    assert coded.tobytes() == payload
    assert lens3 == tuple(int(z[f"mapped{p}"].size) for p in range(3))
    pinned = torch.empty(len(payload), dtype=torch.uint8).pin_memory().numpy()
    assert tm.encodeMapped(coder, out=pinned)[0].tobytes() == payload   # into page-locked memory
    with pytest.raises(PgrcMatchError) as e:
        tm.encodeMapped(coder, out=np.empty(len(payload) - 1, np.uint8))
    assert e.value.code == E_PARAM
    tm._ck(_lib.lib.pgrc_mem_set_src_ascii(tm._h, tm._src.ctypes.data_as(C.c_void_p), tm._src.size))   # a new source forgets the slots
    with pytest.raises(PgrcMatchError) as e:
        tm.encodeMapped(coder)
    assert e.value.code == E_STATE
    tm.close()

    offs = [z[f"off{p}"] for p in range(3)]
    lns = [z[f"len{p}"] for p in range(3)]
    dec = PgRCDecoder(100, device=0)
    dec.restoreMatchedPgs(vu.joined_mapped(z), lens3, hq.size, offs, lns, True)
    plain = dec.text().tobytes()
    dec.set_mapped_text_coded(coder, payload, lens3, hq.size, offs, lns, True)
    assert dec.text_lengths() == tuple(t.size for t in texts)
    assert dec.text().tobytes() == plain == b"".join(t.tobytes() for t in texts)
    with pytest.raises(PgrcMatchError) as e:
        dec.set_mapped_text_coded(coder, payload[:-1], lens3, hq.size, offs, lns, True)       # a payload cut by one byte
    assert e.value.code == E_PARAM
    with pytest.raises(PgrcMatchError) as e:
        dec.text(0, 1)
    assert e.value.code == E_STATE                                      # ... leaves no text
    dec.set_mapped_text_coded(coder, payload, lens3, hq.size, offs, lns, True)
    assert dec.text().tobytes() == plain
    dec.close()
