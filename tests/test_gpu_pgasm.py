"""The assembly of a pseudogenome from the overlap graph on the device (pgrc_asm_run; pgrc_amd/csrc/pgasm.hip): device == the
reference-made fixtures byte for byte -- text, off, orgIdx and the logged numbers; device == tests/pgasm_util's literal loops
on generated cases around the wave and text-tile sizes, in both alphabets, at read lengths around the 32-symbol work item and
at the ends of the range, with and without an index mapping, with overlaps of one and two bytes, and on the special shapes
(a pair, a two-cycle, a self-link, a chain and a cycle that need 17 jumping passes, singles only, duplicates only, a
million mixed reads); the text in pieces across tile borders; the packed text handed to a matcher; every refusal, each
followed by a good run on the same context; a text longer than 2^32; and a small run after a large one on one context."""
import ctypes as C

import numpy as np
import pytest

import pgasm_util as pa
from pgrc_amd import MatchContext, PgAssembler, PgrcMatchError
from pgrc_amd import _lib
from pgrc_amd._lib import lib
from test_pgasm_oracle import FIXTURES, NUMBERS, case_name, load_case

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = 1, 6
TILE = 8192                 # AS_TILE of pgasm.hip: text bytes of one block


def run_case(asm, c, mapping=None):
    got = asm.run(c["rows"], c["next_read"], c["overlap"], c["L"], c["symbols"], mapping)
    got["text"] = asm.text()
    return got


def assert_equal(got, want, what=""):
    for k in NUMBERS:
        assert int(got[k]) == int(want[k]), (what, k, int(got[k]), int(want[k]))
    for k, dt in (("text", np.uint8), ("off", np.uint16), ("org_idx", np.uint32)):
        g, w = got[k], np.asarray(want[k])
        assert g.dtype == np.dtype(dt) and g.size == w.size, (what, k, g.dtype, g.size, w.size)
        assert g.tobytes() == w.astype(dt).tobytes(), (what, k)


def split_reads(rng, R):
    """R reads as chains, cycles and singles"""
    chains, cycles, left = [], [], R
    while left > 0:
        n = int(min(left, rng.integers(1, max(2, R // 3 + 1))))
        (cycles if rng.random() < 0.3 else chains).append(n)
        left -= n
    return chains, cycles


@pytest.mark.parametrize("path", FIXTURES, ids=case_name)
def test_reference_fixtures(path):
    fx = load_case(path)
    asm = PgAssembler(device=0)
    got = asm.run(fx["rows"], fx["next_read"], fx["overlap"], int(fx["L"]), int(fx["symbols"]))
    got["text"] = asm.text()
    assert_equal(got, fx, case_name(path))
    t = asm.timing()
    assert t["bytes_down"] == 6 * fx["rows"].shape[0] and t["passes_rank"] >= 1
    asm.close()


@pytest.mark.parametrize("symbols", [4, 5])
@pytest.mark.parametrize("L", [1, 31, 32, 33, 150, 255])
def test_generated_cases_equal_the_literal_loops(L, symbols):
    asm = PgAssembler(device=0)
    fill = -(-TILE // L)                                    # singles that fill one text tile
    for k, R in enumerate([1, 2, 63, 64, 65, fill - 1, fill + 1]):
        rng = np.random.default_rng(100 * L + 10 * symbols + k)
        if R >= fill - 1:
            chains, cycles, singles = [], [], R             # the tile border falls between two reads
        else:
            chains, cycles = split_reads(rng, R)
            singles = 0
        c = pa.make_case(seed=7 * L + k, L=L, symbols=symbols, chains=chains, cycles=cycles, singles=singles, dup=0.1 if k % 2 else 0.0,
                         mean_shift=max(1, L // 5), n_share=0.03, ov_dtype=np.uint16 if (k + L) % 2 else np.uint8)
        mapping = rng.permutation(R).astype(np.uint32) if k % 2 else None
        want = pa.literal(c["reads"], c["next_read"], c["overlap"], mapping)
        assert_equal(run_case(asm, c, mapping), want, (L, symbols, R))
    # the same tile sizes with chains: borders inside reads, shifts of 0 at a border
    for k, R in enumerate([fill - 1, fill + 1]):
        c = pa.make_case(seed=90 + k, L=L, symbols=symbols, chains=[R // 2, R - R // 2 - 3], cycles=[3], dup=0.2, mean_shift=max(1, L // 3), n_share=0.03)
        assert_equal(run_case(asm, c), pa.literal(c["reads"], c["next_read"], c["overlap"]), (L, symbols, R, "chains"))
    asm.close()


SHAPES = {
    "pair": dict(L=20, chains=[2]),
    "two_cycle": dict(L=20, cycles=[2]),
    "self_link": dict(L=20, cycles=[1]),
    "chain_70000": dict(L=20, chains=[70000], mean_shift=3, dup=0.05),
    "cycle_70000": dict(L=20, cycles=[70000], mean_shift=3, dup=0.05),
    "all_singles": dict(L=33, singles=3000, symbols=5, n_share=0.02),
    "duplicates_only": dict(L=150, chains=[700], dup=1.0),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    c = pa.make_case(seed=11, **SHAPES[name])
    want = pa.literal(c["reads"], c["next_read"], c["overlap"])
    asm = PgAssembler(device=0)
    assert_equal(run_case(asm, c), want, name)
    t = asm.timing()
    if name == "chain_70000":
        # 17 passes bring the tail to the head when every pass reads what the pass before wrote (ceil(log2(69999))), one more
        # finds nothing to do; a pass in place may read what it has just written and get there sooner
        assert 2 <= t["passes_rank"] <= 18 and want["cycles"] == 0
    if name == "cycle_70000":
        assert t["passes_cycles"] == 18 and want["cycles"] == 1             # ceil(log2(R + 1)) + 1: a cycle never runs out
    if name == "duplicates_only":
        assert want["pg_len"] == 150 and int((want["off"] == 0).sum()) == 700
    if name in ("two_cycle", "self_link"):
        assert want["cycles"] == 1 and want["components"] == (1 if name == "two_cycle" else 0)
    asm.close()


def test_a_million_mixed_reads_then_a_small_case_on_the_same_context():
    rng = np.random.default_rng(5)
    chains = rng.integers(500, 1500, size=890).tolist()
    cycles = rng.integers(1, 3000, size=60).tolist()
    singles = 1_000_000 - sum(chains) - sum(cycles)
    assert singles > 1000
    c = pa.make_case(seed=5, L=24, chains=chains, cycles=cycles, singles=singles, dup=0.05, mean_shift=5)
    mapping = rng.permutation(1_000_000).astype(np.uint32)
    asm = PgAssembler(device=0)
    got = run_case(asm, c, mapping)
    want = pa.literal(c["reads"], c["next_read"], c["overlap"], mapping)
    assert want["cycles"] == 60
    assert_equal(got, want, "1M")
    # nothing of the large run survives a small one
    small = pa.make_case(seed=6, L=150, symbols=5, chains=[40, 3], cycles=[5], singles=2, n_share=0.02)
    assert_equal(run_case(asm, small), pa.literal(small["reads"], small["next_read"], small["overlap"]), "small after large")
    p, n = asm.text_device()
    assert p and n == asm.pg_len
    with pytest.raises(PgrcMatchError) as e:
        asm.text(asm.pg_len - 1, 2)
    assert e.value.code == E_PARAM
    asm.close()


def test_text_in_pieces_across_tile_borders():
    c = pa.make_case(seed=21, L=100, chains=[700, 500], cycles=[50], singles=20, mean_shift=30)
    asm = PgAssembler(device=0)
    got = run_case(asm, c)
    whole = got["text"]
    assert whole.size > 3 * TILE
    assert_equal(got, pa.literal(c["reads"], c["next_read"], c["overlap"]))
    for first, n in [(0, 1), (TILE - 1, 2), (TILE - 5, TILE + 10), (2 * TILE, TILE), (TILE + 1, 2 * TILE - 1), (whole.size - 7, 7), (5, 0), (whole.size, 0)]:
        assert asm.text(first, n).tobytes() == whole[first:first + n].tobytes(), (first, n)
    import torch
    pinned = torch.empty(whole.size, dtype=torch.uint8).pin_memory()
    view = pinned.numpy()
    assert asm.text(3, whole.size - 3, out=view).tobytes() == whole[3:].tobytes()
    asm.close()


def pack2(text):
    """the 2-bit layout of pgrc_match_set_pg_packed_device: 16 symbols per word, the first in the lowest bits"""
    lut = np.zeros(256, dtype=np.uint32)
    for k, ch in enumerate(b"ACGT"):
        lut[ch] = k
    codes = np.zeros((text.size + 15) // 16 * 16, dtype=np.uint32)
    codes[:text.size] = lut[text]
    return (codes.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint32)


@pytest.mark.parametrize("extra", [0, 5])
def test_packed_text_goes_straight_to_a_matcher(extra):
    c = pa.make_case(seed=31 + extra, L=50, chains=[200, 117 + extra], cycles=[30], singles=5, mean_shift=9)
    asm = PgAssembler(device=0)
    got = run_case(asm, c)
    words = asm.packed_device()
    assert words and asm.packed_device() == words           # made once
    ctx = MatchContext(150, 38, 3, 0, "c", device=0)
    ctx.set_pg_packed_device(words, int(got["pg_len"]))
    assert ctx.export_pg(0).tobytes() == pack2(got["text"]).tobytes()
    ctx.close()
    five = pa.make_case(seed=33, L=50, symbols=5, chains=[20], singles=2)
    run_case(asm, five)
    with pytest.raises(PgrcMatchError) as e:
        asm.packed_device()
    assert e.value.code == E_PARAM
    asm.close()


def raw_run(asm, c, **change):
    """pgrc_asm_run on the arrays of case `c` with fields of the input changed -> (code, result struct)"""
    rows = np.ascontiguousarray(c["rows"])
    nx = np.ascontiguousarray(c["next_read"], dtype=np.uint32)
    ov = np.ascontiguousarray(c["overlap"])
    f = dict(struct_size=C.sizeof(_lib.AsmInput), read_len=c["L"], symbols=c["symbols"], overlap_width=ov.dtype.itemsize, n_reads=nx.size - 1,
             packed_rows=rows.ctypes.data, next_read=nx.ctypes.data, overlap=ov.ctypes.data, index_mapping=None)
    f.update(change)
    inp = _lib.AsmInput(**f)
    res = _lib.AsmResult()
    res.pg_len = 77                                           # (must be cleared)
    return lib.pgrc_asm_run(asm._h, C.byref(inp), C.byref(res)), res


def broken_cases():
    good = pa.make_case(seed=41, L=31, symbols=5, chains=[30, 12], cycles=[6], singles=4, mean_shift=6, n_share=0.02, shuffle=False)
    # (ids in walk order: reads 1..30 and 31..42 are the chains, 43..48 the cycle, 49..52 the singles)
    out = []

    def variant(name, **arrays):
        c = dict(good)
        for k, v in arrays.items():
            a = good[k].copy()
            v(a)
            c[k] = a
        out.append((name, c, {}))

    for name, change in [("in NULL", None), ("struct_size", dict(struct_size=8)), ("read_len 0", dict(read_len=0)), ("read_len 256", dict(read_len=256)),
                         ("symbols 3", dict(symbols=3)), ("width 3", dict(overlap_width=3)), ("width 0", dict(overlap_width=0)), ("no reads", dict(n_reads=0)),
                         ("2^32 - 1 reads", dict(n_reads=0xFFFFFFFF)), ("rows NULL", dict(packed_rows=None)), ("next NULL", dict(next_read=None)),
                         ("overlap NULL", dict(overlap=None))]:
        out.append((name, good, change))
    variant("successor above R", next_read=lambda a: a.__setitem__(52, 53))
    variant("two predecessors", next_read=lambda a: a.__setitem__(49, 2), overlap=lambda a: a.__setitem__(49, 0))
    variant("overlap above L", overlap=lambda a: a.__setitem__(3, 32))
    variant("overlap without a successor", overlap=lambda a: a.__setitem__(50, 1))
    variant("a false overlap", overlap=lambda a: a.__setitem__(5, a[5] + 1 if a[5] < 31 else 30))
    variant("a false overlap at the link that is cut", overlap=lambda a: a.__setitem__(48, a[48] + 1 if a[48] < 31 else 30))
    variant("a byte of 125", rows=lambda a: a.__setitem__((50, 4), 125))
    variant("a pad digit", rows=lambda a: a.__setitem__((51, 10), a[51, 10] + 1))      # L = 31: the last byte holds one symbol
    return good, out


def test_every_refusal_leaves_the_context_usable():
    good, cases = broken_cases()
    for name, c, _ in cases:
        if name.startswith("a false overlap"):
            assert not pa.links_are_real(c["reads"], c["next_read"], c["overlap"]), name
    want = pa.literal(good["reads"], good["next_read"], good["overlap"])
    assert want["cycles"] == 1 and want["cuts"] == [48]
    asm = PgAssembler(device=0)
    assert_equal(run_case(asm, good), want)
    res = _lib.AsmResult()
    assert lib.pgrc_asm_run(asm._h, None, None) == E_PARAM
    for name, c, change in cases:
        if change is None:
            res = _lib.AsmResult()
            res.pg_len = 77
            code = lib.pgrc_asm_run(asm._h, None, C.byref(res))
        else:
            code, res = raw_run(asm, c, **change)
        assert code == E_PARAM, name
        assert lib.pgrc_asm_last_error(asm._h), name
        assert bytes(res) == bytes(_lib.AsmResult()), name                      # cleared
        buf = np.zeros(4, dtype=np.uint8)
        assert lib.pgrc_asm_get_text(asm._h, 0, 1, buf.ctypes.data_as(C.c_void_p)) == E_STATE, name       # no text installed
        p, n = C.c_void_p(), C.c_uint64()
        assert lib.pgrc_asm_text_device(asm._h, C.byref(p), C.byref(n)) == E_STATE, name
        assert lib.pgrc_asm_packed_device(asm._h, C.byref(p)) == E_STATE, name
        t = _lib.AsmTiming(C.sizeof(_lib.AsmTiming))
        assert lib.pgrc_asm_get_timing(asm._h, C.byref(t)) == E_STATE, name
        assert_equal(run_case(asm, good), want, "after " + name)
    asm.close()


def test_a_text_longer_than_two_to_the_32():
    L, rb = 255, 64
    rng = np.random.default_rng(77)
    n_single = (2 ** 32 + 3000) // L + 1
    distinct = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(4099, L))]
    drows = pa.pack_rows(distinct, 4)
    tail = pa.make_case(seed=78, L=L, chains=[3, 4, 5], mean_shift=40)          # 12 reads, ids permuted
    R = n_single + 12
    rows = np.empty((R, rb), dtype=np.uint8)
    for at in range(0, n_single, 4099):
        n = min(4099, n_single - at)
        rows[at:at + n] = drows[:n]
    rows[n_single:] = tail["rows"]
    nx = np.zeros(R + 1, dtype=np.uint32)
    ov = np.zeros(R + 1, dtype=np.uint8)
    nx[n_single + 1:] = np.where(tail["next_read"][1:] != 0, tail["next_read"][1:] + n_single, 0)
    ov[n_single + 1:] = tail["overlap"][1:]
    asm = PgAssembler(device=0)
    got = asm.run(rows, nx, ov, L, 4)
    want_tail = pa.literal(tail["reads"], tail["next_read"], tail["overlap"])
    pg_len = n_single * L + want_tail["pg_len"]
    assert got["pg_len"] == pg_len > 2 ** 32 + 3000
    assert (got["cycles"], got["components"], got["singles"]) == (0, 3, n_single)

    def singles_text(first_read, n):                                            # the literal loop over singles: their rows, one after the other
        idx = (np.arange(first_read, first_read + n) % 4099)
        lit = pa.literal(distinct[idx], np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint8))
        return lit["text"]

    assert asm.text(0, 10 * L).tobytes() == singles_text(0, 10).tobytes()
    r0 = 2 ** 32 // L - 8                                                       # reads around byte 2^32
    assert r0 * L < 2 ** 32 - 1000 and (r0 + 16) * L > 2 ** 32 + 1000
    assert asm.text(r0 * L, 16 * L).tobytes() == singles_text(r0, 16).tobytes()
    end = np.concatenate([singles_text(n_single - 5, 5), want_tail["text"]])
    assert asm.text(pg_len - end.size, end.size).tobytes() == end.tobytes()
    assert np.array_equal(got["org_idx"][-12:], want_tail["org_idx"] + n_single)
    assert np.array_equal(got["off"][-11:], want_tail["off"][1:]) and got["off"][-12] == L and got["off"][0] == 0
    assert np.array_equal(got["org_idx"][:n_single:100003], np.arange(0, n_single, 100003, dtype=np.uint32))
    assert (got["off"][1:n_single] == L).all()
    asm.close()
