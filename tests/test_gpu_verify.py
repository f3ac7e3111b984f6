"""The verifier on the device (include/pgrc_verify.h, pgrc_amd/verify.py) against tests/verify_util.py, field for field, in both
kinds: jobs matched and exported on the device in SE, PE and ORD order and plain jobs of L = 1, 8, 16 and 255; item counts
round the scan block and past its carry round; every perturbation of the source that a word-wise key or compare could miss;
the source as pageable and page-locked rows, one row a call, odd pieces, one file ahead of the other, and as FASTQ text cut
inside every line; the refusals; pairs that collide under keys of the test's choosing and under keys cut to 8 and 20 bits;
and a round trip at 2 M reads against the input reads themselves.  The expected rows are decode_util's restatement."""
import ctypes as C

import numpy as np
import pytest

import decode_util as du
import prim_util as pu
import verify_util as vu
from pgrc_amd import _lib, MatchContext, PgRCDecoder, PgrcMatchError, Verifier, synth
from test_gpu_decode import add_lists, decoder, device_job

pytestmark = pytest.mark.gpu

KINDS = (vu.IN_ORDER, vu.MULTISET)
E_PARAM, E_STATE = 1, 6


# ---------------------------------------------------------------------------------------------- jobs
def open_job(dc, mode, pair=False):
    """-> (decoder with the order set, the rows of its files without '\\n' as decode_util writes them)"""
    if mode == "SE":
        dec = decoder(dc)
        dec.set_order(0)
        files = (du.write_se(dc),)
    elif mode == "PE":
        dec = decoder(dc)
        ro = np.asarray(dc["rl_idx_order"], np.uint32)
        dec.set_order(1, ro.size, rl_idx_order=ro, rev_compl_pair_file=pair)
        files = du.write_pe(dc, ro, pair)
    else:
        dec = decoder(dc, dc["ord_lists"])
        op = np.asarray(dc["org2pos"], np.uint64)
        dec.set_order(2, op.size, org_idx_to_pos=op, paired=pair, rev_compl_pair_file=pair)
        files = du.write_ord(dict(dc, lists=dc["ord_lists"]), op, paired=pair, pair_file=pair)
    return dec, [np.ascontiguousarray(f[:, :-1]) for f in files]


def plain_job(L, n, seed, two_files=False, pos=None):
    """random text, a list of positions, no mismatches: one file in SE order, or two in PE order"""
    rng = np.random.default_rng(seed)
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=max(n, 1) * L + 64)].copy()
    text[rng.integers(0, text.size, text.size // 50)] = ord("N")
    if pos is None:
        pos = rng.integers(0, text.size - L + 1, size=n)
    dc = {"L": L, "text": text, "lists": [{"text_base": 0, "n": n, "pos": np.asarray(pos, np.uint64)}]}
    if two_files:
        dc["rl_idx_order"] = rng.permutation(n).astype(np.uint32)
    return open_job(dc, "PE" if two_files else "SE")


def verify(dec, kind, src_files, feed=None, library=None):
    v = Verifier(dec, kind, library=library)
    try:
        if feed is not None:
            feed(v, src_files)
        else:
            for f, rows in enumerate(src_files):
                v.add_rows(f, rows)
        return v.finish()
    finally:
        v.close()


def check(dec, dec_files, src_files, kinds=KINDS, feed=None):
    out = []
    for kind in kinds:
        got = verify(dec, kind, src_files, feed)
        assert got == vu.reference(kind, src_files, dec_files), (kind, got)
        out.append(got)
    return out


# ---------------------------------------------------------------------------------------------- perturbations
def other(b):
    return ord("A") if b != ord("A") else ord("C")


def perturbations(files):
    """(name, source files) for every perturbation the job's shape allows"""
    n, L, F = min(f.shape[0] for f in files), files[0].shape[1], len(files)
    out = []

    def edit(name, fn):
        src = [f.copy() for f in files]
        src = fn(src) or src
        out.append((name, [np.ascontiguousarray(s) for s in src]))
    for r in sorted({0, n // 2, n - 1}):
        for c in sorted({0, L - 1}):
            for f in range(F):
                def flip(s, r=r, c=c, f=f):
                    s[f][r, c] = other(s[f][r, c])
                edit(f"flip row {r} byte {c} file {f}", flip)
    a, b = 1, n - 2

    def swap(s):
        for f in range(F):
            s[f][[a, b]] = s[f][[b, a]]
    edit("two rows swapped", swap)
    edit("one row dropped", lambda s: [np.delete(x, n // 3, axis=0) for x in s])

    def copy_row(s):
        s[0][a] = s[0][b]
    edit("a row replaced by a copy of another", copy_row)

    def all_n(s):
        s[F - 1][n // 2] = ord("N")
    edit("a row of all N", all_n)
    edit("one row longer", lambda s: [np.concatenate([s[0], s[0][:1]])] + s[1:])
    edit("one row shorter", lambda s: [s[0][:-1]] + s[1:])
    if F == 2:
        def mates(s):
            s[0][a], s[1][a] = files[1][a], files[0][a]
        edit("mates exchanged between the files", mates)
        p = np.concatenate([[b], np.delete(np.arange(n), b)])
        edit("a whole pair moved", lambda s: [x[p] for x in s])
        edit("file 1 one row shorter", lambda s: [s[0], s[1][:-1]])
    return out


_cases = {}


def device_case(L, pair):
    if (L, pair) not in _cases:
        case, res, pg_st, org_st = device_job(40 + L + pair, L, pair, n=3000, n_with_n=80)
        _cases[(L, pair)] = du.decode_case(case, res, pg_st, org_st, pair=pair)
    return _cases[(L, pair)]


@pytest.mark.parametrize("mode", ["SE", "PE", "ORD"])
@pytest.mark.parametrize("L,pair", [(37, False), (150, True), (250, False)])
def test_device_jobs_under_every_perturbation(L, pair, mode):
    dec, files = open_job(device_case(L, pair), mode, pair)
    assert len(files) == (1 if mode == "SE" or (mode == "ORD" and not pair) else 2)
    # AUTO: what the archive mode promises
    got = verify(dec, 0, files)
    assert got["kind"] == (vu.IN_ORDER if mode == "ORD" else vu.MULTISET) and got == vu.reference(got["kind"], files, files) and got["ok"]
    for r in check(dec, files, files):
        assert r["ok"]
    for name, src in perturbations(files):
        for r in check(dec, files, src):
            assert not r["ok"] or not name.startswith(("flip", "one row", "file 1")), name
    dec.close()


@pytest.mark.parametrize("L", [1, 8, 16, 255])
@pytest.mark.parametrize("two_files", [False, True])
def test_plain_jobs_under_every_perturbation(L, two_files):
    dec, files = plain_job(L, 130, 7 * L + two_files, two_files)
    check(dec, files, files)
    for name, src in perturbations(files):
        check(dec, files, src)
    dec.close()


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193])
def test_item_counts_round_the_scan_block(n):
    dec, files = plain_job(16, n, n)
    assert all(r["ok"] for r in check(dec, files, files))
    if n:
        src = files[0].copy()
        src[n - 1, 15] = other(src[n - 1, 15])
        for r in check(dec, files, [src]):
            assert not r["ok"] and (r["first_mismatch_row"] if r["kind"] == vu.IN_ORDER else r["first_source_unmatched"]) == n - 1
    two, tfiles = plain_job(16, 2 * n + 1, n + 1, two_files=True)       # n + 1 and n rows: n items
    assert tfiles[0].shape[0] == n + 1 and tfiles[1].shape[0] == n
    assert all(r["ok"] for r in check(two, tfiles, tfiles))
    dec.close()
    two.close()


def test_past_the_scan_carry_round():
    """1 048 577 items of L = 16: several sort tiles, the scans' carry round; rows that occur many times"""
    n = 1_048_577
    rng = np.random.default_rng(5)
    dec, files = plain_job(16, n, 5, pos=rng.integers(0, 200_000, size=n))
    src = files[0][rng.permutation(n)]
    got = verify(dec, vu.MULTISET, [src])
    assert got["ok"] and got["salts_used"] == 1 and got["n_source"] == [n, 0]
    src[n - 1, 15] = other(src[n - 1, 15])
    assert verify(dec, vu.MULTISET, [src]) == vu.verify_multiset([src], files)
    src = files[0].copy()
    src[[0, n - 1], 0] = [other(src[0, 0]), other(src[n - 1, 0])]
    assert verify(dec, vu.IN_ORDER, [src]) == vu.verify_in_order([src], files)
    dec.close()


def test_many_copies_of_one_read():
    """5000 copies on both sides, and 4999 against 5000: one run of the sorted union holds them all"""
    pos = np.concatenate([np.zeros(5000, np.int64), 16 + np.arange(50) * 16])
    dec, files = plain_job(16, pos.size, 9, pos=pos)
    rng = np.random.default_rng(9)
    src = files[0][rng.permutation(pos.size)]
    check(dec, files, [src])
    assert verify(dec, vu.MULTISET, [src])["ok"]
    less = np.delete(files[0], 17, axis=0)
    got, = check(dec, files, [less], kinds=(vu.MULTISET,))
    assert (got["decoded_unmatched"], got["first_decoded_unmatched"], got["source_unmatched"]) == (1, 4999, 0)
    more = np.concatenate([files[0][:3], files[0]])
    got, = check(dec, files, [more], kinds=(vu.MULTISET,))
    assert (got["source_unmatched"], got["first_source_unmatched"]) == (3, 5000)
    dec.close()


# ---------------------------------------------------------------------------------------------- forms of the source
def pinned_copy(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).pin_memory()
    pinned_copy.keep.append(t)
    return t.numpy()


pinned_copy.keep = []


@pytest.mark.parametrize("kind", KINDS)
def test_rows_in_every_form(kind):
    dec, files = plain_job(150, 1201, 3, two_files=True)
    want = vu.reference(kind, files, files)
    assert want["ok"] and want["n_source"] == [601, 600]
    src = [f.copy() for f in files]
    src[1][77, 149] = other(src[1][77, 149])
    bad = vu.reference(kind, src, files)

    def pinned(v, s):
        for f, rows in enumerate(s):
            v.add_rows(f, pinned_copy(rows))

    def by_address(v, s):
        for f, rows in enumerate(s):
            v.add_rows(f, rows.ctypes.data, rows.shape[0])

    def one_row_a_call(v, s):
        for r in range(max(x.shape[0] for x in s)):
            for f, rows in enumerate(s):
                if r < rows.shape[0]:
                    v.add_rows(f, rows[r])

    def odd_pieces(v, s):
        vu.feed_rows(v, 0, s[0], [1, 7, 130, 3])
        vu.feed_rows(v, 1, s[1], [129, 2, 61], take=pinned_copy)

    def file_1_ahead(v, s):
        v.add_rows(1, s[1][:100])
        for a in range(0, 601, 100):
            v.add_rows(0, s[0][a: a + 100])
            v.add_rows(1, s[1][100 + a: 200 + a])
    for feed in (pinned, by_address, one_row_a_call, odd_pieces, file_1_ahead):
        assert verify(dec, kind, files, feed) == want, feed.__name__
        assert verify(dec, kind, src, feed) == bad, feed.__name__
    pinned_copy.keep.clear()
    dec.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("two_files", [False, True])
def test_fastq_text_in_pieces(kind, two_files):
    L, n = 37, 41
    dec, files = plain_job(L, n * (2 if two_files else 1), 21, two_files)
    texts = [vu.fastq_text(f, id_len=12 + 3 * k, seed=k) for k, f in enumerate(files)]
    want = vu.reference(kind, files, files)
    rec = 12 + 1 + L + 1 + 2 + L + 1
    # a piece size that is no divisor of the record: the cuts walk through all four lines of a record
    for sizes in ([rec + 7], [13], [5 * rec - 1, 3], [10 ** 6]):
        v = Verifier(dec, kind)
        assert vu.feed_fastq(v, texts[0], texts[1] if two_files else None, sizes) == sum(f.shape[0] for f in files)
        assert v.finish() == want and want["ok"], sizes
        v.close()
    cuts = set()
    for sizes in ([rec + 7], [13]):
        c = vu.cut_points(texts[0].size, sizes)
        cuts |= {("id" if x % rec < 13 else "read" if x % rec < 14 + L else "plus" if x % rec < 16 + L else "qual") for x in c[1:-1]}
    assert cuts == {"id", "read", "plus", "qual"}
    # a last line without a newline; a changed read
    src = [f.copy() for f in files]
    src[-1][n // 2, L - 1] = other(src[-1][n // 2, L - 1])
    texts = [vu.fastq_text(f, seed=k, last_newline=False) for k, f in enumerate(src)]
    v = Verifier(dec, kind)
    vu.feed_fastq(v, texts[0], texts[1] if two_files else None, [997])
    assert v.finish() == vu.reference(kind, src, files)
    v.close()
    dec.close()


@pytest.mark.parametrize("kind", KINDS)
def test_fastq_pair_files_of_unequal_length(kind):
    L, n = 16, 30
    dec, files = plain_job(L, 2 * n, 33, two_files=True)
    # the second file three records short: the reference's iteration stops at the first exhausted file, and so does the source
    short = [files[0], files[1][: n - 3]]
    texts = [vu.fastq_text(f, seed=k) for k, f in enumerate(short)]
    v = Verifier(dec, kind)
    took = vu.feed_fastq(v, texts[0], texts[1], [10 ** 6])
    assert took == 2 * (n - 3) + 1
    seen = [files[0][: n - 2], files[1][: n - 3]]
    assert v.finish() == vu.reference(kind, seen, files)
    v.close()
    dec.close()


def test_refusals_leave_the_handle_usable():
    dec, files = plain_job(16, 40, 2)
    two, tfiles = plain_job(16, 80, 2, two_files=True)
    for kind in KINDS:
        v, v2 = Verifier(dec, kind), Verifier(two, kind)
        v.add_rows(0, files[0][:10])
        v2.add_rows(0, tfiles[0][:10])
        text = vu.fastq_text(files[0][10:])

        def refused(fn, code=E_PARAM, word=""):
            with pytest.raises(PgrcMatchError) as e:
                fn()
            assert e.value.code == code and word in str(e.value)
        refused(lambda: v.add_rows(1, files[0][:1]), word="file 1")
        refused(lambda: v2.add_rows(2, files[0][:1]), word="file 2")
        refused(lambda: v.add_rows(0, 0, 5), word="NULL")
        refused(lambda: v.add_fastq(text, text), word="pair_text on a job of one file")
        refused(lambda: v2.add_fastq(text), word="needs pair_text")
        longer = vu.fastq_text(np.concatenate([files[0][:2], files[0][:2, :8]], axis=1))
        refused(lambda: v.add_fastq(longer, final=True), word="variable length")
        refused(lambda: v.add_fastq(text[: text.size - 20], final=True), word="ends inside a record")
        r = _lib.VerifyResult()
        assert v._lib.pgrc_verify_finish(v._h, C.byref(r)) == E_PARAM            # struct_size 0: not counted as the finish
        # ... and the handles still answer
        assert v.add_fastq(text, final=True)[2] == 30
        v2.add_rows(0, tfiles[0][10:])
        v2.add_rows(1, tfiles[1])
        assert v.finish() == vu.reference(kind, files, files) and v2.finish() == vu.reference(kind, tfiles, tfiles)
        refused(v.finish, E_STATE, "after finish")
        refused(lambda: v.add_rows(0, files[0][:1]), E_STATE)
        assert v.timing()["bytes_up"] > 0
        v.close()
        v2.close()
    # a job without an order
    raw = PgRCDecoder(16, device=0)
    raw.set_text(np.frombuffer(b"ACGT" * 20, np.uint8))
    with pytest.raises(PgrcMatchError) as e:
        Verifier(raw)
    assert e.value.code == E_STATE and "no order" in str(e.value)
    with pytest.raises(PgrcMatchError) as e:
        Verifier(dec, 3)
    assert e.value.code == E_PARAM
    for d in (dec, two, raw):
        d.close()


def test_item_limit_of_the_multiset_kind():
    """0x7FFFF800 items: one more row is refused before anything is allocated for it (the count alone decides)"""
    dec, files = plain_job(1, 5, 1)
    v = Verifier(dec, vu.MULTISET)
    big = np.zeros(16, np.uint8)
    with pytest.raises(PgrcMatchError) as e:
        v.add_rows(0, big.ctypes.data, 0x7FFFF800 + 1)
    assert e.value.code == E_PARAM and "0x7FFFF800" in str(e.value)
    v.add_rows(0, files[0])
    assert v.finish()["ok"]
    v.close()
    dec.close()


def test_an_allocation_that_fails_names_its_bytes():
    """the largest source the MULTISET kind takes, at L = 255: 548 GB of rows that no part holds; the store is asked for
    before a byte of the caller's is read, the refusal names the bytes, and the handle goes on"""
    dec, files = plain_job(255, 5, 1)
    v = Verifier(dec, vu.MULTISET)
    v.add_rows(0, files[0][:2])
    big = np.zeros(16, np.uint8)
    with pytest.raises(PgrcMatchError) as e:
        v.add_rows(0, big.ctypes.data, 0x7FFFF800 - 2)
    assert e.value.code == 4 and str((0x7FFFF800 * 255) + 16) in str(e.value)       # PGRC_E_ALLOC
    v.add_rows(0, files[0][2:])
    assert v.finish() == vu.verify_multiset(files, files)
    v.close()
    dec.close()


# ---------------------------------------------------------------------------------------------- collisions
def selftest_lib():
    L = pu.lib()
    vp, u64 = C.c_void_p, C.c_uint64
    L.pgrc_selftest_verify_match.argtypes = [vp, vp, vp, u64, vp, vp, u64, C.c_uint32, C.POINTER(u64)]
    L.pgrc_selftest_verify_mask_next_begin.argtypes = [C.c_uint32]
    L.pgrc_selftest_verify_mask_next_begin.restype = None
    return _lib.bind_verify(L)


def match_under_keys(st, keys_s, items_s, keys_d, items_d):
    L = selftest_lib()
    ks, kd = np.ascontiguousarray(keys_s, np.uint64), np.ascontiguousarray(keys_d, np.uint64)
    a, b = np.ascontiguousarray(items_s, np.uint8), np.ascontiguousarray(items_d, np.uint8)
    B = a.shape[1] if a.size else b.shape[1]
    out = (C.c_uint64 * 6)()
    st._check(L.pgrc_selftest_verify_match(st.h, pu._ptr(ks), pu._ptr(a), ks.size, pu._ptr(kd), pu._ptr(b), kd.size, B, out), "verify_match")
    return tuple(int(x) for x in out)


def test_pairs_under_keys_of_the_tests_choosing():
    st = pu.SelfTest()
    x, y = np.frombuffer(b"ACGTACGTACGTACGTACG", np.uint8), np.frombuffer(b"ACGTACGTACGTACGTACT", np.uint8)     # differ in the last byte
    one = [7, 7]
    assert match_under_keys(st, one, [x, y], one, [y, x]) == (0, 2, 0, 0, vu.NONE64, vu.NONE64)       # undecided, never matched
    assert match_under_keys(st, one, [x, y], one, [x, y]) == (2, 0, 0, 0, vu.NONE64, vu.NONE64)
    # few keys over many items of 1 .. 41 bytes: every run mixes unrelated items
    rng = np.random.default_rng(4)
    for B in (1, 7, 8, 9, 41):
        pool = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, size=(60, B))]
        s, d = pool[rng.integers(0, 60, 5000)], pool[rng.integers(0, 60, 4097)]
        ks, kd = vu.hash_items(s, 0, 3), vu.hash_items(d, 0, 3)
        assert match_under_keys(st, ks, s, kd, d) == vu.pair_under_keys(ks, s, kd, d), B
    st.close()


def test_keys_cut_to_8_bits_stay_undecided():
    L = selftest_lib()
    dec, files = plain_job(16, 1000, 12, pos=np.arange(1000) * 16)
    assert np.unique(files[0], axis=0).shape[0] == 1000
    src = files[0][np.random.default_rng(12).permutation(1000)]
    L.pgrc_selftest_verify_mask_next_begin(8)
    got = verify(dec, vu.MULTISET, [src], library=L)
    assert not got["ok"] and got["undecided"] > 0 and got["salts_used"] == 3
    assert got["source_unmatched"] == 0 and got["decoded_unmatched"] == 0
    # the cut was taken by that begin and does not last
    got = verify(dec, vu.MULTISET, [src], library=L)
    assert got["ok"] and got["salts_used"] == 1
    dec.close()


def test_a_collision_under_20_bits_is_settled_by_the_next_salt():
    L = selftest_lib()
    seed = vu.find_collision_seed()
    rows, perm = vu.collision_case(seed)
    dc = {"L": vu.COLLISION_L, "text": rows.reshape(-1).copy(), "lists": [{"text_base": 0, "n": vu.COLLISION_N, "pos": np.arange(vu.COLLISION_N, dtype=np.uint64) * vu.COLLISION_L}]}
    dec, files = open_job(dc, "SE")
    assert np.array_equal(files[0], rows)
    L.pgrc_selftest_verify_mask_next_begin(vu.COLLISION_BITS)
    got = verify(dec, vu.MULTISET, [rows[perm]], library=L)
    assert got["ok"] and got["salts_used"] == 2 and got["undecided"] == 0
    dec.close()


# ---------------------------------------------------------------------------------------------- at scale
def test_round_trip_at_2m_reads_against_the_input_reads():
    """2 M reads x 100 bp: MatchContext -> export in Pg order (over an old list with an entry every 200 symbols, as every HQ
    list reaches the Pg end) -> the SE job, verified as a multiset against the input reads themselves and the old list's
    windows; once more with ten reads altered"""
    L, G, n = 100, 40_000_000, 2_000_000
    g = synth.pg_params(G, seed=13, tandem_every=4)
    pg = synth.pg_host(g)
    reads = synth.reads_host(g, pg, synth.reads_params(n, L, seed=13, n_with_n=10_000))
    lpos = np.arange(0, G - L + 1, 200, dtype=np.int64)
    if lpos[-1] != G - L:
        lpos = np.append(lpos, G - L)
    h = lpos.size
    ctx = MatchContext(L, 38, 33, 0, "c", device=0)
    ctx.set_pg_ascii(pg)
    ctx.set_reads_ascii(reads)
    ctx.init_results()
    ctx.run(True)
    _, _, mism, _, matched = ctx.get_results()
    assert matched > n // 2
    st = ctx.export_pg_order(None, np.diff(lpos, prepend=0).astype(np.uint8), (n + np.arange(h)).astype(np.uint32))
    ctx.close()
    um = np.flatnonzero(mism == 255)
    dec = PgRCDecoder(L, device=0)
    dec.set_text(np.concatenate([pg, reads[um].reshape(-1)]))
    add_lists(dec, [{"text_base": 0, "n": st["org_idx"].size, "off": st["off"], "rc": st["rev_comp"], "mis_cnt": st["mis_cnt"],
                     "mis_sym": st["mis_sym"], "mis_off": st["mis_rev_off"], "form": 1},
                    {"text_base": G, "n": um.size, "pos": np.arange(um.size, dtype=np.uint64) * L}])
    dec.set_order(0)
    assert dec.row_count(0) == n + h
    src = np.concatenate([reads, pg[lpos[:, None] + np.arange(L)]])
    got = verify(dec, 0, [src])
    assert got["kind"] == vu.MULTISET and got["ok"] and got["n_source"] == [n + h, 0] == got["n_decoded"] and got["undecided"] == 0
    # ten reads altered in their last symbol to a lower-case letter, which no row of the job holds: each of them finds no partner,
    # and each leaves one row of the job without one
    hit = np.arange(10) * 199_999 + 7
    src[hit, L - 1] = ord("a")
    got = verify(dec, vu.MULTISET, [src])
    assert not got["ok"] and got["undecided"] == 0 and got["salts_used"] == 1
    assert (got["source_unmatched"], got["first_source_unmatched"], got["decoded_unmatched"]) == (10, 7, 10)
    dec.close()
