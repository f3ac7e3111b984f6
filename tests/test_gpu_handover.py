"""The hand-over -- what puts the text and the reads on the device -- held to numpy, exactly: pack.hip's kernels driven directly
through libpgrc_selftest.so, and the host packer, the upload loop append_rows and the multi-device all-gather through the product
library, whose state afterwards pgrc_selftest_reads_state reads back.  The references are
tests/handover_util.py's, which tests/test_handover_reference.py holds to the oracle on the CPU.  Every buffer a kernel writes
is pre-filled: what lies outside the addressed part must come back as fill, and the guard zones untouched."""
import functools

import numpy as np
import pytest

import handover_util as hu
import prim_util as pu
from util import assert_same_results, gpu_match, make_inputs

pytestmark = pytest.mark.gpu

E_SYMBOL = 5
N_TOTAL, STRIDE = 700, 704
MI = 1 << 20


@pytest.fixture(scope="module")
def ho():
    h = hu.HandOver(0)
    yield h
    h.close()


@pytest.fixture(scope="module", autouse=True)
def drop_cached_inputs():
    yield
    read_block.cache_clear()
    text_case.cache_clear()


# ---------------------------------------------------------------------------------------------- the kernels: text
TEXT_SIZES = list(range(1, 81)) + [4095, 4096, 4097, 65543]


def test_text_pack_and_reverse_complement_kernels(ho):
    """k_pack_ascii and k_revcomp at every G in 1..80 (every G mod 16 below, at and above one word, the whole-word loads and the
    tail loop), around 4096 and at 65 543: the words, the partial last word of both strands, a clear error flag"""
    rng = np.random.default_rng(16)
    for G in TEXT_SIZES:
        pg = hu.ASCII[rng.integers(0, 4, G, dtype=np.uint8)]
        want = hu.pack_text(pg)
        words, err, guards = ho.pack_text(pg)
        assert guards == 3, f"G {G}: guard zones written (bit 0 words, bit 1 flag): {guards:#x}"
        assert err == 0, f"G {G}: error flag {err} on a clean text"
        assert np.array_equal(words, want), f"G {G}: packed words differ at {np.flatnonzero(words != want)[:8]}"
        rc, guards = ho.revcomp(want, G)
        want_rc = hu.revcomp_text(pg)
        assert guards == 1, f"G {G}: the zone after the reverse complement was written"
        assert np.array_equal(rc, want_rc), f"G {G}: reverse complement differs at {np.flatnonzero(rc != want_rc)[:8]}"


def test_text_pack_kernel_flags_a_symbol_outside_acgt(ho):
    """... at the first position, the last one and the last of a word (16 k - 1), whichever path packs that word; 'N', a lower-case
    letter and a byte that shares its code bits with a letter"""
    rng = np.random.default_rng(17)
    for G in (1, 15, 16, 17, 47, 48, 80, 4097):
        pg = hu.ASCII[rng.integers(0, 4, G, dtype=np.uint8)]
        for at in sorted({0, G - 1} | {16 * k - 1 for k in range(1, G // 16 + 1)}):
            for sym in (hu.N, ord("a"), ord("A") | 0x80):
                bad = pg.copy()
                bad[at] = sym
                _, err, guards = ho.pack_text(bad)
                assert guards == 3 and err == 1, f"G {G}: symbol {sym} at {at}: flag {err}, guards {guards:#x}"


# ---------------------------------------------------------------------------------------------- the kernels: reads
def n_patterns(L, rng):
    """N positions of the hand-made rows of a block: none, 1, 4, 5 and L N's; at symbol 0, at L - 1, on both sides of the word edge
    15 | 16 and of the base-5 byte edge 2 | 3"""
    pats = [[], [0], [L - 1], [15], [16], [15, 16], [2], [3], [2, 3], [0, 1, 2, 3], [L - 4, L - 3, L - 2, L - 1], [0, 15, 16, L - 1],
            [0, 1, 2, 3, 4], [L - 5, L - 4, L - 3, L - 2, L - 1], list(range(L)),
            sorted(rng.choice(L, min(4, L), replace=False)), sorted(rng.choice(L, min(5, L), replace=False)), [L // 2]]
    return [sorted({p for p in pat if 0 <= p < L}) for pat in pats]


@functools.lru_cache(maxsize=4)
def read_block(L, kind):
    """257 rows of L symbols and their reference: the patterns above first, then random rows of which a fifth hold a few N's"""
    rng = np.random.default_rng(1000 * kind + L)
    rows = hu.ASCII[rng.integers(0, 4, (257, L), dtype=np.uint8)]
    pats = []
    if kind != 4:
        pats = n_patterns(L, rng)
        for r, pat in enumerate(pats):
            rows[r, pat] = hu.N
        more = len(pats) + np.flatnonzero(rng.random(257 - len(pats)) < 0.2)
        for r in more:
            rows[r, rng.choice(L, min(L, int(rng.integers(1, 7))), replace=False)] = hu.N
    st = hu.read_state(rows)
    return rows, hu.rows_of(rows, kind), st, max(len(pats), 1)


def check_block(ho, kind, L, lo, count, first):
    """rows [lo, lo + count) of the block as reads [first, first + count) of N_TOTAL"""
    rows, host, st, _ = read_block(L, kind)
    words, nflag, npos, err, guards = ho.pack_reads(kind, host[lo:lo + count], first, L, N_TOTAL, STRIDE)
    what = f"kind {kind} L {L} count {count} first {first} (row {lo})"
    assert guards == 15, f"{what}: guard zones written (bit 0 words, 1 nflag, 2 npos, 3 error flag): {guards:#x}"
    assert err == 0, f"{what}: error flag {err}"
    want = np.full(words.shape, pu.fill_of(np.uint32)[0], dtype=np.uint32)
    want[:, first:first + count] = st["words"][:, lo:lo + count]
    if not np.array_equal(words, want):
        w, r = (int(x[0]) for x in np.nonzero(words != want))
        raise AssertionError(f"{what}: word {w} of column {r}: got {words[w, r]:#010x}, want {want[w, r]:#010x}")
    want_flag = np.zeros(N_TOTAL, dtype=np.uint8)
    want_flag[first:first + count] = st["flag"][lo:lo + count]
    assert np.array_equal(nflag, want_flag), f"{what}: flags differ at {np.flatnonzero(nflag != want_flag)[:8]}"
    want_npos = pu.fill_of(np.uint32, N_TOTAL).copy()                      # untouched but for the reads flagged 3
    sel = first + np.flatnonzero(st["flag"][lo:lo + count] == 3)
    want_npos[sel] = st["npos"][sel - first + lo]
    assert np.array_equal(npos, want_npos), f"{what}: position words differ at {np.flatnonzero(npos != want_npos)[:8]}"


@pytest.mark.parametrize("kind", [0, 4, 5])
def test_read_kernels_at_every_read_length(ho, kind):
    """k_pack_reads_ascii (0), k_repack_reads_ref (4) and k_unpack_reads_acgnt (5), each followed by k_npos_rows as append_rows
    does, at every L in 1..255 -- every L mod 16 of the word layout, mod 4 of the ACGT bytes, mod 3 of the base-5 bytes --, with a
    block of 257 rows (two thread blocks from two words on) and of one row, put at the start and in the middle of 700 reads
    with a stride of 704.  The single row walks through the hand-made N patterns as L grows.
    The launchers cap their grids at 262 144 blocks; reaching that takes gigabytes of rows and is not tested."""
    for L in range(1, 256):
        npat = read_block(L, kind)[3]
        for first in (0, 300):
            check_block(ho, kind, L, 0, 257, first)
            check_block(ho, kind, L, (L + first) % npat, 1, first)


@pytest.mark.parametrize("L", [1, 3, 16, 17, 150, 255])
def test_read_kernels_flag_a_bad_symbol(ho, L):
    """a byte of 125 or more in an ACGNT row and a byte outside ACGNT in an ASCII row set the error flag, wherever they stand;
    no byte of an ACGT row can"""
    rows, _, _, _ = read_block(L, 0)
    rows = rows[:40]
    for at in sorted({0, L - 1, L // 2, min(15, L - 1), min(16, L - 1)}):
        for sym in (ord("a"), ord("n"), 0, ord("A") | 0x80):
            bad = rows.copy()
            bad[17, at] = sym
            assert ho.pack_reads(0, bad, 0, L, N_TOTAL, STRIDE)[3:] == (1, 15), f"ASCII rows, L {L}: symbol {sym} at {at}"
    packed = hu.rows_of(rows, 5)
    for b in sorted({0, packed.shape[1] - 1, packed.shape[1] // 2}):
        for v in (125, 200, 255):
            bad = packed.copy()
            bad[23, b] = v
            assert ho.pack_reads(5, bad, 300, L, N_TOTAL, STRIDE)[3:] == (1, 15), f"ACGNT rows, L {L}: byte {v} at {b}"
        ok = packed.copy()
        ok[23, b] = 124                                 # TTT: the largest code
        assert ho.pack_reads(5, ok, 300, L, N_TOTAL, STRIDE)[3:] == (0, 15), f"ACGNT rows, L {L}: byte 124 at {b}"
    anything = np.random.default_rng(L).integers(0, 256, (40, (L + 3) // 4), dtype=np.uint8)
    words, nflag, _, err, guards = ho.pack_reads(4, anything, 0, L, N_TOTAL, STRIDE)
    assert (err, guards) == (0, 15) and not nflag.any()
    codes = np.zeros((40, L), dtype=np.uint8)
    for i in range(L):
        codes[:, i] = (anything[:, i // 4] >> (2 * (3 - i % 4))) & 3
    assert np.array_equal(words[:, :40], hu.read_words(codes))


def test_nrows_ascii_kernel(ho):
    """k_nrows_ascii_acgnt: a shuffled index list with repeats at a few read lengths, and 70 000 rows of L = 250, whose
    count * L passes the grid's cap of 65 536 blocks of 256 threads: the grid-stride loop.  (The other launchers cap at 262 144
    blocks, which takes gigabytes of rows to reach: not tested.)"""
    rng = np.random.default_rng(3)
    for L in (1, 2, 3, 4, 100, 151, 255):
        rows = read_block(L, 5)[0]
        idx = rng.integers(0, rows.shape[0], 600)
        got, guards = ho.nrows_ascii(hu.rows_of(rows, 5), idx, L)
        assert guards == 1 and np.array_equal(got, rows[idx]), f"L {L}"
    rows = read_block(250, 5)[0]
    idx = rng.integers(0, rows.shape[0], 70_000)
    assert idx.size * 250 > 65536 * 256
    got, guards = ho.nrows_ascii(hu.rows_of(rows, 5), idx, 250)
    assert guards == 1 and np.array_equal(got, rows[idx])


# ---------------------------------------------------------------------------------------------- contexts: the reads
def rows_with_n(n, L, seed, n_at, none_in=None):
    """n random rows; N's in the rows n_at (1 to 6 of them per row, by the row's number) and in 1 % of the others, but in no row
    of the range none_in"""
    rng = np.random.default_rng(seed)
    rows = hu.ASCII[rng.integers(0, 4, (n, L), dtype=np.uint8)]
    pick = np.union1d(np.flatnonzero(rng.random(n) < 0.01), np.asarray(n_at, dtype=np.int64))
    if none_in is not None:
        pick = pick[(pick < none_in[0]) | (pick >= none_in[1])]
    for r in pick:
        rows[r, rng.choice(L, 1 + int(r) % 6, replace=False)] = hu.N
    return rows


def check_state(ho, ctx, rows, multi, what):
    want = hu.read_state(rows)
    shards = ho.reads_state(ctx, multi=multi)
    assert len(shards) == (2 if multi else 1)
    assert shards[0]["lo"] == 0 and shards[-1]["hi"] == rows.shape[0] and all(a["hi"] == b["lo"] for a, b in zip(shards, shards[1:]))
    for r, s in enumerate(shards):
        lo, hi = s["lo"], s["hi"]
        w = f"{what}, shard {r} [{lo}, {hi})"
        assert s["n"] == hi - lo and s["stride"] >= s["n"] and s["nw"] == want["words"].shape[0], w
        assert np.array_equal(s["words"][:, :s["n"]], want["words"][:, lo:hi]), w
        flag = want["flag"][lo:hi]
        assert np.array_equal(s["flag"], flag), f"{w}: flags differ at {np.flatnonzero(s['flag'] != flag)[:8]}"
        three = flag == 3
        if three.any():
            assert s["npos"] is not None and np.array_equal(s["npos"][three], want["npos"][lo:hi][three]), w
        idx = np.flatnonzero(flag)
        assert s["n_nreads"] == idx.size and s["n_many"] == int((flag == 1).sum()), w
        assert np.array_equal(s["nidx"], idx), f"{w}: the side list's indexes"
        assert np.array_equal(s["nascii"], rows[lo:hi][idx]), f"{w}: the side list's rows"
    return shards


def chunk_rows(L, kind):
    """append_rows' rows per staging chunk at PGRC_UPLOAD_CHUNK_MB=1"""
    rb = L if kind == 0 else (L + 3) // 4 if kind == 4 else (L + 2) // 3
    return max(1024, (MI // rb) & ~1023)


def edge_rows(n, chr_, multi):
    """both sides of every chunk edge of a set of n rows handed over in one call -- of both shards' where it is split in two
    (multi.hip's shard_range: even halves) --, and the set's first and last row"""
    starts = [0, ((n + 1) // 2 + 1) & ~1] if multi else [0]
    return sorted({0, n - 1} | {e + d for s in starts for e in range(s, n, chr_) for d in (-1, 0) if 0 <= e + d < n})


def handed_over(ho, multi, L, kmax, sets, what):
    """a fresh context, the sets [(ASCII rows, kind)] handed over in their format, the state held to the reference"""
    from pgrc_amd import MatchContext
    ctx = MatchContext(L, 38, kmax, 0, "c", **({"devices": [0, 0]} if multi else {}))
    if len(sets) == 1 and sets[0][1] == 0:
        ctx.set_reads_ascii(sets[0][0])
    elif len(sets) == 1 and sets[0][1] == 4:
        ctx.set_reads_packed(hu.rows_of(sets[0][0], 4), sets[0][0].shape[0])
    else:
        ctx.set_reads_packed_sets([(hu.rows_of(rows, kind), rows.shape[0], kind) for rows, kind in sets])
    shards = check_state(ho, ctx, np.concatenate([rows for rows, _ in sets]), multi, what)
    ctx.close()
    return shards


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("gap", [False, True])
def test_reads_in_several_staging_chunks(ho, monkeypatch, multi, gap):
    """append_rows' loop over staging chunks of 1 MiB (two staging areas in turn, first = up_next + off, the N rows collected chunk
    by chunk): set_reads_ascii with 9000 rows of L = 255 (chunks of 4096 rows), set_reads_packed with 90 000 ACGT rows of
    L = 100 (40 960), set_reads_packed_sets with 60 000 ACGT rows (26 624) and then 45 000 ACGNT rows (20 480) of L = 150, and
    with that ACGNT set alone: three chunks each, the last one partial.  N reads in every chunk and on both sides of every chunk
    edge; gap: none in the middle chunk.  multi: the same through two shards on one device, each of which holds its range (and
    cuts its own chunks)."""
    monkeypatch.setenv("PGRC_UPLOAD_CHUNK_MB", "1")

    def rows_for(n, L, kind, seed, per_chunk, with_n=True):
        c = chunk_rows(L, kind)
        assert (c, -(-n // c)) == (per_chunk, 3) and n % c
        return rows_with_n(n, L, seed, edge_rows(n, c, multi) if with_n else [], ((c, 2 * c) if gap else None) if with_n else (0, n))
    handed_over(ho, multi, 255, 5, [(rows_for(9000, 255, 0, 1, 4096), 0)], "ASCII rows")
    for s in handed_over(ho, multi, 100, 2, [(rows_for(90_000, 100, 4, 2, 40960, with_n=False), 4)], "ACGT rows"):
        assert s["n_nreads"] == 0 and s["npos"] is None         # (an ACGT set allocates no position array)
    nset = rows_for(45_000, 150, 5, 3, 20480)
    handed_over(ho, multi, 150, 3, [(rows_for(60_000, 150, 4, 4, 26624, with_n=False), 4), (nset, 5)], "an ACGT set, then an ACGNT set")
    handed_over(ho, multi, 150, 3, [(nset, 5)], "ACGNT rows")


def test_streamed_hand_over_in_several_chunks(ho, monkeypatch):
    """match_streamed with staging chunks of 1 MiB: an ACGT set of five chunks (40 960 rows of L = 100 each, the last one
    partial), which the upload loop does not wait for between chunks, and an ACGNT set of two (30 720).  The read state
    afterwards equals the reference, the results the plain run's."""
    from pgrc_amd import MatchContext
    L, n_n = 100, 31_000
    n_lq = 4 * chunk_rows(L, 4) + 5000
    assert chunk_rows(L, 4) == 40960 and chunk_rows(L, 5) == 30720
    pg, reads = make_inputs(400_000, n_lq + n_n, L, seed=77, n_with_n=n_n)
    plain = gpu_match("c", pg, reads, 38, 2, 0, n_nset=n_n)
    monkeypatch.setenv("PGRC_UPLOAD_CHUNK_MB", "1")
    ctx = MatchContext(L, 38, 2, 0, "c")
    ctx.set_pg_ascii(pg)
    ctx.prepare_index(True)
    pos, rc, mism, hist, matched = ctx.match_streamed([(hu.rows_of(reads[:n_lq], 4), n_lq, 4), (hu.rows_of(reads[n_lq:], 5), n_n, 5)])
    assert_same_results({"pos": pos, "rc": rc, "mism": mism, "hist": hist, "matched": matched}, plain, "streamed in 1 MiB chunks")
    check_state(ho, ctx, reads, False, "streamed")
    check_state(ho, plain["ctx"], reads, False, "plain, one chunk")
    ctx.close()


# ---------------------------------------------------------------------------------------------- contexts: the text
@functools.lru_cache(maxsize=1)
def text_case(G, seed=0):
    pg = hu.random_text(G, 4000 + seed + G % 1000)
    out = (pg, hu.pack_text(pg), hu.revcomp_text(pg))
    for a in out:
        a.setflags(write=False)
    return out


def text_context(pg):
    from pgrc_amd import MatchContext
    ctx = MatchContext(100, 38, 2, 0, "c")
    ctx.set_pg_ascii(pg)
    return ctx


# five chunks of 1 Mi symbols with a partial last word; three whole chunks of 2 Mi (a text below 4 Mi symbols does not take the
# host path, so exactly three chunks of 1 Mi never run it: that size goes through both packers all the same); four whole chunks
HOST_PACK_CASES = [(MI, 4 * MI + 16 * 3 + 5), (2 * MI, 6 * MI), (MI, 3 * MI), (MI, 4 * MI)]


@pytest.mark.parametrize("chunk,G", HOST_PACK_CASES)
def test_host_packer_in_several_chunks(monkeypatch, chunk, G):
    """pgrc_match_pack_pg_slice's host branch with PGRC_TEST_PACK_CHUNK: the pinned pair used again from chunk 2 on (ordered by
    `copied` and `packed[k]`), the off / 16 word offsets, 1, 3 and 16 packing threads; against the kernel packer
    (PGRC_HOST_PACK=0) and numpy, on both strands"""
    pg, want, want_rc = text_case(G)
    monkeypatch.setenv("PGRC_TEST_PACK_CHUNK", str(chunk))
    for host_pack, threads in (("0", "1"), ("1", "1"), ("1", "3"), ("1", "16")):
        monkeypatch.setenv("PGRC_HOST_PACK", host_pack)
        monkeypatch.setenv("PGRC_HOST_THREADS", threads)
        ctx = text_context(pg)
        fw, rc = ctx.export_pg(0), ctx.export_pg(1)
        ctx.close()
        what = f"G {G} chunk {chunk} host_pack {host_pack} threads {threads}"
        assert np.array_equal(fw, want), f"{what}: forward words differ at {np.flatnonzero(fw != want)[:8]}"
        assert np.array_equal(rc, want_rc), f"{what}: reverse complement differs at {np.flatnonzero(rc != want_rc)[:8]}"


@pytest.mark.parametrize("threads", ["1", "3", "16"])
def test_host_packer_refuses_a_bad_symbol_in_any_chunk(monkeypatch, threads):
    from pgrc_amd import MatchContext, PgrcMatchError
    G = 4 * MI + 16 * 3 + 5
    pg = text_case(G)[0]
    monkeypatch.setenv("PGRC_TEST_PACK_CHUNK", str(MI))
    monkeypatch.setenv("PGRC_HOST_PACK", "1")
    monkeypatch.setenv("PGRC_HOST_THREADS", threads)
    for at in (5, 2 * MI + MI // 3, G - 1):              # chunk 0, chunk 2, the last symbol (chunk 4, the tail of a word)
        bad = pg.copy()
        bad[at] = hu.N
        ctx = MatchContext(100, 38, 2, 0, "c")
        with pytest.raises(PgrcMatchError) as e:
            ctx.set_pg_ascii(bad)
        assert e.value.code == E_SYMBOL, f"'N' at {at}: {e.value}"
        ctx.close()
    ctx = text_context(pg)                               # ... and the clean text is taken afterwards
    assert np.array_equal(ctx.export_pg(0), text_case(G)[1])
    ctx.close()


REAL_G = 3 * 32 * MI + 16 * 5 + 7


def test_host_packer_at_the_real_chunk_size():
    """four chunks of 32 Mi symbols, the last one 87 symbols: the text set and exported, no index and no run"""
    pg, want, want_rc = text_case(REAL_G)
    ctx = text_context(pg)
    assert np.array_equal(ctx.export_pg(0), want)
    assert np.array_equal(ctx.export_pg(1), want_rc)
    ctx.close()


def test_every_shard_holds_the_whole_text(ho):
    """export_pg reads shard 0; the text of the other shard is what allgather_text made of the slices, each packed at the word
    offset r * sw of its own buffer"""
    from pgrc_amd import MatchContext
    pg, want, _ = text_case(REAL_G)
    ctx = MatchContext(100, 38, 2, 0, "c", devices=[0, 0])
    ctx.set_pg_ascii(pg)
    shards = ho.reads_state(ctx, multi=True, text=True)
    assert len(shards) == 2
    for r, s in enumerate(shards):
        assert np.array_equal(s["text"], want), f"shard {r}: words differ at {np.flatnonzero(s['text'] != want)[:8]}"
    assert np.array_equal(ctx.export_pg(0), want)
    ctx.close()


def test_pack_pg_slice_at_a_word_offset():
    import torch
    from pgrc_amd import MatchContext
    pg, want, _ = text_case(REAL_G)
    off = 12345
    buf = torch.full((off + want.size + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    ctx = MatchContext(100, 38, 2, 0, "c")
    ctx.pack_pg_slice(pg, buf.data_ptr() + 4 * off)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[off:off + want.size], want)
    assert (got[:off] == 0x5A5A5A5A).all() and (got[off + want.size:] == 0x5A5A5A5A).all(), "words outside the slice were written"
    ctx.close()


@pytest.mark.parametrize("G", [1000 + 5, 65536 + 15, 300_001])
def test_set_pg_packed_device_masks_the_last_word(G):
    """a source on the device whose last word has garbage above symbol G - 1: the text reads as zero there, on both strands"""
    import torch
    from pgrc_amd import MatchContext
    pg, want, want_rc = text_case(G, seed=1)
    src = want.copy()
    src[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(2 * (G % 16))
    assert src[-1] != want[-1]
    dev = torch.from_numpy(src.view(np.int32)).to("cuda:0")
    ctx = MatchContext(100, 38, 2, 0, "c")
    ctx.set_pg_packed_device(dev.data_ptr(), G)
    assert np.array_equal(ctx.export_pg(0), want)
    assert np.array_equal(ctx.export_pg(1), want_rc)
    ctx.close()
