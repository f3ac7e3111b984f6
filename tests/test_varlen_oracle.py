"""The restatements of the reference's variable-length DNA coder in tests/varlen_util.py, held to what the reference itself
wrote (tests/golden/varlen_*.npz): the serial loop and the parse as folded tile maps both give the reference's payload on
every fixture and agree on generated texts around the tile's edges and on runs of one symbol, decode gives the text back,
and every recorded book has the properties pgrc_varlen_create demands.  No GPU."""
import numpy as np
import pytest

import varlen_util as vu

FIXTURES = vu.load_fixtures()
CASES = [(name, text, bid, stream) for name, text, streams in FIXTURES for bid, stream in sorted(streams.items())]


def book_of(bid):
    for _, _, streams in FIXTURES:
        if bid in streams:
            return vu.parse_stream(streams[bid])[2]
    raise KeyError(bid)


def test_fixtures_present():
    names = {name for name, _, _ in FIXTURES}
    want = {n for n, _, _, size in vu.TEXT_CASES if size >= 4} | {"pgmap_hq_lq_n", "pgmap_empty_n", "pgmap_short_hq", "pgmap_low_complexity", "pgmap_rc_chains"}
    assert want <= names
    for name, _, streams in FIXTURES:
        assert set(streams) == ({0} if name.startswith("pgmap_") else set(vu.BOOK_IDS)), name


@pytest.mark.parametrize("bid", vu.BOOK_IDS)
def test_books_have_what_create_demands(bid):
    book = book_of(bid)
    book.check()
    assert bytes(book.symbols) == b"%ACGNT" and [s & 7 for s in book.symbols] == [5, 1, 3, 7, 6, 4]
    filled = [c for c in book.codes if c]
    assert len(set(filled)) == len(filled) and len(book.codes) == 256
    # the same book behind every stream of that id
    for _, _, streams in FIXTURES:
        if bid in streams:
            assert vu.parse_stream(streams[bid])[2].raw == book.raw


@pytest.mark.parametrize("name,text,bid,stream", CASES, ids=[f"{c[0]}-{c[2]}" for c in CASES])
def test_restatements_give_the_references_payload(name, text, bid, stream):
    mode, got_id, book, payload = vu.parse_stream(stream)
    assert (mode, got_id) == (0, bid)
    assert vu.encode_serial(book, text) == payload
    par, exit_off, tiles = vu.encode_parallel(book, text, 64)
    assert par == payload and tiles == (text.size + 63) // 64
    assert vu.decode(book, payload) == text.tobytes()


def generated_texts():
    rng = np.random.default_rng(2024)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    alphabet = np.frombuffer(b"ACGTN%", np.uint8)
    out = []
    for tiles in (1, 2, 3, 5, 8):
        for d in range(-4, 5):                              # a tile multiple +- 0..4
            n = 64 * tiles + d
            out.append(acgt[rng.integers(0, 4, size=n)])
            out.append(alphabet[rng.integers(0, 6, size=n)])
            out.append(np.full(n, ord("ACGTN%"[(tiles + d) % 6]), np.uint8))   # a run of one symbol: entries that never merge
    for n in list(range(0, 10)) + [63, 64, 65, 127, 128, 129, 255, 257, 1000, 4097]:
        out.append(alphabet[rng.integers(0, 6, size=n)])
        t = acgt[rng.integers(0, 4, size=n)].copy()
        if n:
            t[rng.integers(0, n, size=max(n // 50, 1))] = ord("%")
        out.append(t)
    for s in b"ACGTN%":
        out.append(np.full(300, s, np.uint8))
    return out


@pytest.mark.parametrize("bid", vu.BOOK_IDS)
def test_serial_and_parallel_agree_on_generated_texts(bid):
    book = book_of(bid)
    texts = generated_texts()
    assert len(texts) >= 180
    for t in texts:
        want = vu.encode_serial(book, t)
        for tile in (64, 4):
            got, exit_off, _ = vu.encode_parallel(book, t, tile)
            assert got == want, (bid, t.size, tile)
        assert vu.decode(book, want) == t.tobytes()


def test_the_map_operator():
    rng = np.random.default_rng(3)
    maps = [tuple(int(x) for x in rng.integers(0, 4, size=4)) for _ in range(37)]
    assert vu.compose(vu.MAP_IDENTITY, maps[0]) == maps[0] == vu.compose(maps[0], vu.MAP_IDENTITY)
    a, b, c = maps[:3]
    assert vu.compose(vu.compose(a, b), c) == vu.compose(a, vu.compose(b, c))
    run, want = vu.MAP_IDENTITY, []
    for m in maps:
        want.append(run)
        run = vu.compose(run, m)
    assert vu.exclusive_fold(maps) == want
    # the identity in the packed form of scanops.h
    assert sum(e << (2 * e) for e in range(4)) == 0b11100100 == vu.source_constants()["SCO_MAP4_IDENTITY"]
