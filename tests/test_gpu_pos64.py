"""Everything that consumes a matcher's 64-bit positions, at positions that do not fit 32 bits, without a matcher run: the
export of the matches (export.hip: the scan of the old list's offset deltas, the two binary-search merges, the 16-bit
offset arithmetic, k_export_offsets_abs, the word indexing of k_export_mismatches), the mismatch extraction (results.hip,
also per shard: mismatch_streams_from_shards) and the read rebuild over the exported streams.

The text has 2^32 + 3000 symbols and is sparse: all 'A' except a random tail that starts about 1 M symbols below 2^32.
The reads are planted on the host -- positions, strands and mismatch counts are known by construction -- and handed over
with set_results, the two-phase entry point.  Reads at p in the all-'A' head and at p + 2^32 alias under any truncation of
a position to 32 bits.  Every stream of every entry point is compared with the oracle's, every mismatch list with the
oracle's, and the rebuilt rows with the planted reads themselves."""
import numpy as np
import pytest
import torch

import decode_util as du
import export_util as xu
import oracle as orc
from pgrc_amd import MatchContext, PgRCDecoder, PgrcMatchError
from pgrc_amd.decode import PGRC_DECODE_ORD, PGRC_DECODE_SE
from util import _CODE, _COMP

pytestmark = pytest.mark.gpu

L = 150
B = 1 << 32
G = B + 3000
TAIL = (B - 1_000_000) & ~15            # the random tail starts on a 16-symbol boundary
HEAD = 3000                             # the part of the all-'A' region that reads are planted in
NOT_MATCHED = np.uint64(2**64 - 1)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _old_list(rng):
    """offset deltas of 150-250 from position 0 to the text end: it crosses 2^32 and is closed at G - L"""
    off = rng.integers(150, 251, size=(G - L) // 195).astype(np.uint8)
    off[0] = 0                                                     # an entry at position 0
    lpos = np.cumsum(off, dtype=np.int64)
    h = int(np.searchsorted(lpos, G - L, side="right"))
    assert h < off.size                                            # (the deltas drawn do reach the text end)
    return off[:h]


def _plant(rng, pg, pos, rc, k_sub, k_n):
    """reads with k_sub substitutions and k_n N's against the windows at pos, reverse-complemented where rc"""
    n = pos.size
    codes = _CODE[pg[pos[:, None] + np.arange(L)]]
    assert (codes < 4).all()                                       # every window lies in the written parts of the sparse text
    cols = np.argsort(rng.random((n, L)), axis=1)[:, :8]           # 8 distinct offsets per read
    j = np.arange(8)[None, :]
    sub = j < k_sub[:, None]
    rr = np.broadcast_to(np.arange(n)[:, None], cols.shape)
    codes[rr[sub], cols[sub]] = (codes[rr[sub], cols[sub]] + rng.integers(1, 4, size=int(sub.sum()))) & 3
    w = ACGT[codes]
    isn = (j >= k_sub[:, None]) & (j < (k_sub + k_n)[:, None])
    w[rr[isn], cols[isn]] = ord("N")
    return np.where(rc[:, None] != 0, _COMP[w[:, ::-1]], w)


class _World:
    """the sparse text in HBM and on the host, the old list, the planted reads and their results"""

    def __init__(self):
        rng = np.random.default_rng(64)
        # host: the joined text of the round trip -- the pseudogenome, then the unmatched reads (their LQ text); untouched
        # pages of the zeros stay unallocated.  A zero byte stands for the device's code 0, 'A': the checkers only touch
        # the windows of the matched reads, and the windows used in the head are written as 'A'
        n_um = 1500
        self.text = np.zeros(G + n_um * L, dtype=np.uint8)
        self.pg = pg = self.text[:G]
        pg[:HEAD] = ord("A")
        pg[TAIL:] = ACGT[rng.integers(0, 4, size=G - TAIL)]
        # device: 2 bits per symbol, all zero = all 'A', the tail packed into its place
        self.d_pg = torch.zeros((G + 15) // 16 + 64, dtype=torch.int32, device="cuda")
        ctx = MatchContext(L, 38, 50, 0, "c", device=0)
        ctx.pack_pg_slice(pg[TAIL:], self.d_pg.data_ptr() + 4 * (TAIL // 16))
        torch.cuda.synchronize()
        ctx.close()
        # the old list
        off = _old_list(rng)
        h0 = off.size
        case = {"pg": pg, "L": L, "list_off": off, "list_org": np.zeros(h0, np.uint32), "list_rc": np.zeros(h0, np.uint8), "total": 0}
        off = du.close_list(case)["list_off"]
        h = off.size
        lpos = np.cumsum(off, dtype=np.int64)
        assert lpos[-1] == G - L and int((lpos >= B).sum()) >= 10 and h > 20_000_000
        # positions of the matched reads
        old_hi = lpos[(lpos >= B) & (lpos < G - L)]                # old entries above 2^32: a new entry at the same place precedes them
        old_tail = lpos[(lpos >= TAIL) & (lpos < B)]
        alias = np.concatenate([[0, 1, HEAD - L - 1], rng.integers(0, HEAD - L, size=150)])
        rand = rng.integers(TAIL, G - L + 1, size=17_000)
        parts = [np.array([B - 1, B, B - L + 1, G - L, B + 1234, B + 1234], dtype=np.int64), old_hi[:6], old_hi[:2],
                 rng.choice(old_tail, 40, replace=False), alias + B, rand, rng.choice(rand, 300)]   # (300 more positions used twice)
        hi = np.concatenate(parts).astype(np.int64)
        pos = np.concatenate([hi, alias]).astype(np.int64)
        n_m = pos.size
        rc = (rng.random(n_m) < 0.5).astype(np.uint8)
        k_sub = rng.integers(0, 6, size=n_m)
        k_sub[hi.size:] = rng.integers(0, 4, size=alias.size)      # the poly-A reads: 0-3 substitutions
        k_n = np.zeros(n_m, dtype=np.int64)
        with_n = rng.choice(n_m, 400, replace=False)
        k_n[with_n] = rng.integers(1, 4, size=400)
        matched = _plant(rng, pg, pos, rc, k_sub, k_n)
        um = ACGT[rng.integers(0, 4, size=(n_um, L))]
        um[rng.choice(n_um, 60, replace=False), rng.integers(0, L, size=60)] = ord("N")
        # all reads in a random order, so that a read's index says nothing about its position
        n = n_m + n_um
        perm = rng.permutation(n)
        self.reads = np.concatenate([matched, um])[perm]
        self.pos = np.concatenate([pos.astype(np.uint64), np.full(n_um, NOT_MATCHED)])[perm]
        self.rc = np.concatenate([rc, np.zeros(n_um, np.uint8)])[perm]
        self.mism = np.concatenate([(k_sub + k_n).astype(np.uint8), np.full(n_um, 255, np.uint8)])[perm]
        self.n, self.n_um = n, n_um
        self.um = np.flatnonzero(self.mism == 255)
        self.text[G:] = self.reads[self.um].reshape(-1)
        # original indexes: the old list's and the reads' are one permutation of 0 .. total - 1
        total = h + n
        org = rng.permutation(total).astype(np.uint32)
        self.case = {"pg": pg, "reads": self.reads, "L": L, "list_off": off, "list_org": org[:h].copy(),
                     "list_rc": (rng.random(h) < 0.4).astype(np.uint8), "read_org": org[h:].copy(), "total": total}
        self.res = {"pos": self.pos, "rc": self.rc, "mism": self.mism}
        self.order = xu.stable_order(self.pos)
        self.lpos = lpos

    def context(self, devices=None):
        ctx = MatchContext(L, 38, 50, 0, "c", device=0) if devices is None else MatchContext(L, 38, 50, 0, "c", devices=devices)
        ctx.set_pg_packed_device(self.d_pg.data_ptr(), G)
        ctx.set_reads_ascii(self.reads)
        ctx.set_results(self.pos, self.rc, self.mism)
        return ctx


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    del w.d_pg
    torch.cuda.empty_cache()


def _entries(read_org, matched, total, pair_file_mode):
    """xu.original_order_entries without its loop over the original indexes (21 M here): per parity class, all original
    indexes ascending; an unmatched read's index yields nothing, an index outside the read set a filler"""
    owner = np.full(total, 0xFFFFFFFF, dtype=np.uint32)
    owner[read_org] = np.arange(read_org.size, dtype=np.uint32)
    keep = np.ones(total, dtype=bool)
    keep[read_org[~matched]] = False
    o = np.arange(total, dtype=np.uint32)
    if pair_file_mode:
        o = np.concatenate([o[0::2], o[1::2]])
    o = o[keep[o]]
    return owner[o], o


def _same(got, want, what):
    for k in xu.STREAMS:
        assert np.array_equal(got[k], want[k]), (what, k)
    assert got["last_pos"] == want["last_pos"], what


def test_the_case_is_what_it_claims(world):
    """the planted results are true (Hamming distance at the planted place, recomputed from the reads), and the positions
    the issue asks for are there"""
    w = world
    m = np.flatnonzero(w.mism != 255)
    p = w.pos[m].astype(np.int64)
    win = w.pg[p[:, None] + np.arange(L)]
    rd = np.where(w.rc[m, None] != 0, _COMP[w.reads[m][:, ::-1]], w.reads[m])
    assert np.array_equal((rd != win).sum(axis=1).astype(np.uint8), w.mism[m])
    have = set(p.tolist())
    assert {B - 1, B, B - L + 1, G - L} <= have
    assert int((np.unique(p[p >= B], return_counts=True)[1] >= 2).sum()) >= 2             # two reads at one position above 2^32
    assert np.isin(p[p >= B], w.lpos).sum() >= 7                                          # new entries on old entries' positions
    low = p[p < HEAD]
    assert low.size > 100 and np.isin(low + B, p).all()                                   # the alias pairs
    assert (w.reads[m] == ord("N")).any(axis=1).sum() >= 300 and w.um.size == w.n_um
    assert int((w.lpos >= B).sum()) >= 10 and w.lpos[-1] == G - L and w.lpos.size > 20_000_000


def test_export_streams_equal_the_oracle_above_4g(world):
    """export_pg_order (order[] from the host, both offset widths, with and without read_org, the paired-file rule),
    export_entries and export_original_order (both with both values of pair_file_mode and both widths) from one context and from one
    over three shards -- the shards' own mismatch lists -- against the oracle, stream by stream and last_pos"""
    w = world
    case, res, order = w.case, w.res, w.order
    ctxs = {"one": w.context(), "three shards": w.context(devices=[0, 0, 0])}
    lo, lorg, lrc, ro = case["list_off"], case["list_org"], case["list_rc"], case["read_org"]
    # the device-made order is refused at this text size (code 1, PGRC_E_PARAM), and the context still serves the next call
    for name, ctx in ctxs.items():
        with pytest.raises(PgrcMatchError) as e:
            ctx.export_pg_order(None, lo, lorg, lrc, ro)
        assert e.value.code == 1, name
    n_entries = None
    for byte_mode, with_org, pair in [(True, True, False), (True, False, False), (False, True, False), (False, False, False),
                                      (True, True, True)]:
        want = xu.oracle_export_pg_order(case, res, order, pair_file=pair, byte_mode=byte_mode, with_read_org=with_org)
        assert want["last_pos"] == G - L and want["org_idx"].size == lo.size + order.size
        n_entries = want["org_idx"].size
        for name, ctx in ctxs.items():
            got = ctx.export_pg_order(order, lo, lorg, lrc, ro if with_org else None, pair, byte_mode)
            _same(got, want, (name, "pg order", byte_mode, with_org, pair))
    # no RC stream on the old list
    want = xu.oracle_export_pg_order(dict(case, list_rc=None), res, order)
    for name, ctx in ctxs.items():
        _same(ctx.export_pg_order(order, lo, lorg, None, ro), want, (name, "no rc"))
    assert n_entries > 21_000_000
    matched = w.mism != 255
    for pair_mode in (False, True):
        er, eo = _entries(ro, matched, case["total"], pair_mode)
        for byte_mode in (True, False):
            want = xu.oracle_export_entries(case, res, er, eo, pair_file=pair_mode, byte_mode=byte_mode)
            for name, ctx in ctxs.items():
                _same(ctx.export_entries(er, eo, pair_mode, byte_mode), want, (name, "entries", pair_mode, byte_mode))
                got = ctx.export_original_order(ro, case["total"], pair_mode, pair_mode, byte_mode)
                _same(got, want, (name, "original order", pair_mode, byte_mode))
    for ctx in ctxs.values():
        ctx.close()


def test_entry_list_restatement_equals_the_looped_one():
    """_entries against export_util.original_order_entries on a small set"""
    rng = np.random.default_rng(5)
    total, n = 5001, 1700
    ro = rng.permutation(total)[:n].astype(np.uint32)
    matched = rng.random(n) < 0.8
    for pair_mode in (False, True):
        a = _entries(ro, matched, total, pair_mode)
        b = xu.original_order_entries(ro, matched, total, pair_mode, n)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_mismatch_lists_equal_the_oracle_above_4g(world):
    """extract_mismatches (k_extract), in the strand's orientation and under per-read orientation flags, from one context
    and from one over three shards, against the oracle's list of EVERY matched read"""
    w = world
    n = w.n
    cnt = np.where(w.mism == 255, 0, w.mism).astype(np.int64)
    cum_want = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    flag_sets = (None, (w.rc != (w.case["read_org"] & 1)).astype(np.uint8))
    wants = []
    for flags in flag_sets:
        codes, offs = [], []
        for i in np.flatnonzero(cnt):
            rev = w.rc[i] if flags is None else flags[i]
            co, oo = orc.oracle_extract(w.pg, w.pos[i], w.reads[i], w.rc[i], rev, int(cnt[i]))
            codes.append(co)
            offs.append(oo)
        wants.append((np.concatenate(codes), np.concatenate(offs)))
    for devices in (None, [0, 0, 0]):
        ctx = w.context(devices)
        for flags, (codes_want, offs_want) in zip(flag_sets, wants):
            cum, codes, offs = ctx.extract_mismatches(flags)
            assert np.array_equal(cum, cum_want), devices
            assert np.array_equal(codes, codes_want) and np.array_equal(offs, offs_want), (devices, flags is None)
        ctx.close()
    assert int(cum_want[n]) > 30_000


def _rows_of(dec, file, rows_wanted, chunk=1 << 20):
    """rows `rows_wanted` (ascending) of one output file, fetched in pieces; pieces without a wanted row are left out"""
    total = dec.row_count(file)
    out = np.empty((rows_wanted.size, L + 1), dtype=np.uint8)
    for a in range(0, total, chunk):
        lo, hi = np.searchsorted(rows_wanted, [a, a + chunk])
        if hi > lo:
            out[lo:hi] = dec.rows(file, a, min(chunk, total - a))[rows_wanted[lo:hi] - a]
    return out


def test_exported_streams_rebuild_the_planted_reads(world):
    """ground truth, independent of the oracle: the Pg-order and the original-order streams of this text go into the
    decoder; the SE and ORD rows of the reads' entries are the planted reads"""
    w = world
    case = w.case
    lo, lorg, lrc, ro = case["list_off"], case["list_org"], case["list_rc"], case["read_org"]
    ctx = w.context()
    st = ctx.export_pg_order(w.order, lo, lorg, lrc, ro)
    ost = ctx.export_original_order(ro, case["total"])
    ctx.close()
    T = case["total"]
    owner = np.full(T, -1, dtype=np.int64)
    owner[ro] = np.arange(w.n)
    # SE: the HQ entries in list order, then the unmatched reads
    dec = PgRCDecoder(L, device=0)
    dec.set_text(w.text)
    ne = st["org_idx"].size
    dec.add_list(ne, 0, off=st["off"], rev_comp=st["rev_comp"], mis_cnt=st["mis_cnt"], mis_sym=st["mis_sym"],
                 mis_off=st["mis_rev_off"], mis_sym_form=1)
    dec.add_list(w.n_um, G, pos=np.arange(w.n_um, dtype=np.uint64) * L)
    dec.set_order(PGRC_DECODE_SE)
    assert dec.row_count(0) == ne + w.n_um
    r = owner[st["org_idx"].astype(np.int64)]
    at = np.flatnonzero(r >= 0)
    assert at.size == int((w.mism != 255).sum())
    rows = _rows_of(dec, 0, np.concatenate([at, ne + np.arange(w.n_um)]))
    assert np.array_equal(rows[: at.size, :-1], w.reads[r[at]])
    assert np.array_equal(rows[at.size:, :-1], w.reads[w.um])
    assert (rows[:, -1] == ord("\n")).all()
    dec.close()
    # ORD: one row per original index; fillers (the old list's indexes) at position 0
    o2p = np.zeros(T, dtype=np.uint64)
    m = w.mism != 255
    o2p[ro[m]] = w.pos[m]
    o2p[ro[w.um]] = G + np.arange(w.n_um, dtype=np.uint64) * L
    dec = PgRCDecoder(L, device=0)
    dec.set_text(w.text)
    dec.add_list(ost["org_idx"].size, 0, rev_comp=ost["rev_comp"], mis_cnt=ost["mis_cnt"], mis_sym=ost["mis_sym"],
                 mis_off=ost["mis_rev_off"], mis_sym_form=1)
    dec.add_list(w.n_um, G, pos=np.arange(w.n_um, dtype=np.uint64) * L)
    dec.set_order(PGRC_DECODE_ORD, T, org_idx_to_pos=o2p)
    assert dec.row_count(0) == T
    at = np.sort(ro.astype(np.int64))
    rows = _rows_of(dec, 0, at)
    assert np.array_equal(rows[:, :-1], w.reads[owner[at]])
    dec.close()
