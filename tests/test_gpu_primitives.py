"""scanops.h and radix.hip driven directly (libpgrc_selftest.so) and held to numpy, element for element: the sizes around the
scan's block of 4096 and its carry round of 1 048 576, a start other than the identity, non-commuting operators across every
edge, every element type; the sort's tile of 8192, its digit splits, its stability; the segment sort's sizes, overflow list
and both of its ways.  Every buffer a primitive writes has a guard zone that must come back untouched."""
import functools

import numpy as np
import pytest

import prim_util as pu

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
START = (1 << 40) + 12345


@pytest.fixture(scope="module")
def st():
    s = pu.SelfTest(0)
    yield s
    s.close()


def _drawn_sizes():
    return sorted(int(x) for x in np.random.default_rng(4097).integers(4098, pu.SCO_ROUND - 1, 3))


SCAN_SIZES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 8192, 1048575, 1048576, 1048577, 2097153] + _drawn_sizes()


def check_scan(st, kind, x, want, total=None, **kw):
    """out[0 .. n) == want; out[n] == total, or untouched where none is asked for; both guard zones intact"""
    out, guards = st.device_scan(kind, x, **kw)
    n = len(x)
    what = f"kind {kind} n {n} {kw}"
    assert guards == 3, f"{what}: guard zones written (bit 0 out, bit 1 fold scratch): {guards:#x}"
    if not np.array_equal(out[:n], want):
        bad = np.flatnonzero(out[:n] != want)
        raise AssertionError(f"{what}: {bad.size} elements differ, the first at {bad[0]}: got {out[bad[0]]}, want {want[bad[0]]}")
    if total is None:
        assert out[n] == pu.fill_of(out.dtype)[0], f"{what}: out[n] was written"
    else:
        assert out[n] == total, f"{what}: out[n] = {out[n]}, the total is {total}"


@functools.lru_cache(maxsize=2)
def scan_inputs(n):
    rng = np.random.default_rng(1000 + n)
    d = {"u8": rng.integers(0, 256, n, dtype=np.uint8), "u16": rng.integers(0, 1 << 16, n, dtype=np.uint16),
         "u32": rng.integers(0, 1 << 32, n, dtype=np.uint32), "u32small": rng.integers(0, 16, n, dtype=np.uint32),
         "u64": rng.integers(0, (1 << 40) + 1, n, dtype=np.uint64), "u64any": rng.integers(0, 1 << 64, n, dtype=np.uint64),
         "flag": rng.integers(0, 4, n, dtype=np.uint8)}
    for a in d.values():
        a.setflags(write=False)
    return d


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_u32_sum(st, n):
    """pgrc_ps_scan_u32's instance and mem.hip's run-number scans: u32 from u32, uint4 loads on whole blocks with a scalar tail,
    out of place and in place; the second input's sum wraps past 2^32"""
    d = scan_inputs(n)
    for name in ("u32small", "u32"):
        for inclusive in (False, True):
            want = pu.ref_sum(d[name], 32, 0, inclusive)[0].astype(np.uint32)
            for in_place in (False, True):
                check_scan(st, pu.U32_SUM_U32, d[name], want, inclusive=inclusive, in_place=in_place)
    if n >= 15:
        assert int(d["u32"].astype(np.uint64).sum()) >> 32, "the input was meant to wrap"


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_u32_count_of_u8_flags(st, n):
    """the flag scans (MemIsAccept, PmBit0, the pair codings' flags): u8 through a predicate, inclusive count in u32"""
    f = scan_inputs(n)["flag"]
    check_scan(st, pu.U32_FLAG_U8, f, pu.ref_sum((f == 1).astype(np.uint64), 32)[0].astype(np.uint32), inclusive=True)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_u64_sums(st, n):
    """sco_sum_u64 and dec_scan: u8 / u16 / u32 / u64 summed in u64, inclusive and exclusive with the total at n, from 0 and from
    a start other than the identity; the u64 values reach 2^40, so the high word carries across blocks and rounds"""
    d = scan_inputs(n)
    for kind, name in ((pu.U64_SUM_U8, "u8"), (pu.U64_SUM_U16, "u16"), (pu.U64_SUM_U32, "u32"), (pu.U64_SUM_U64, "u64")):
        for start in (0, START):
            inc, total = pu.ref_sum(d[name], 64, start, True)
            exc, _ = pu.ref_sum(d[name], 64, start, False)
            check_scan(st, kind, d[name], exc, total, start=start, inclusive=False, total_at_n=True)
            check_scan(st, kind, d[name], inc, None, start=start, inclusive=True, total_at_n=True)      # (the inclusive form has no out[n])
            check_scan(st, kind, d[name], exc, None, start=start, inclusive=False, total_at_n=False)
            check_scan(st, kind, d[name], inc, None, start=start, inclusive=True, total_at_n=False)
            if not n:                                       # the empty exclusive scan with a total writes out[0] = start, nothing else
                out, guards = st.device_scan(kind, d[name], start=start, inclusive=False, total_at_n=True)
                assert out.tolist() == [start] and guards == 3


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_u64_maximum(st, n):
    """PmMax: the inclusive maximum over u64, values over the whole range"""
    x = scan_inputs(n)["u64any"]
    check_scan(st, pu.U64_MAX, x, pu.ref_max(x, True), inclusive=True)
    if n > 8:                                               # a maximum that sits early: the carried-in value must win in every later block
        y = x.copy()
        y[n // 8] = M64
        check_scan(st, pu.U64_MAX, y, pu.ref_max(y, True), inclusive=True)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_last_valid(st, n):
    """MemLastValid: exclusive, non-commuting, identity 0xFFFFFFFF, which must survive whole empty blocks and whole empty rounds"""
    rng = np.random.default_rng(2000 + n)
    vals = rng.integers(0, 1 << 20, n).astype(np.uint32)
    sparse = np.where(rng.random(n) < 0.01, vals, pu.NONE).astype(np.uint32)
    none = np.full(n, pu.NONE, dtype=np.uint32)
    first_block = none.copy()
    head = min(n, pu.SCO_EPB)
    first_block[:head] = np.where(rng.random(head) < 0.05, vals[:head], pu.NONE)
    if n:
        first_block[rng.integers(0, head)] = 77             # (at least one)
    for x in (sparse, none, first_block):
        check_scan(st, pu.U32_LAST_VALID, x, pu.ref_last_valid(x, False), inclusive=False)
    check_scan(st, pu.U32_LAST_VALID, sparse, pu.ref_last_valid(sparse, False), inclusive=False, in_place=True)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_segmented_sum(st, n):
    """the 12-byte (int64, set) element of the pair-position decoder: three-word shuffles and LDS slots, operator order across
    every edge"""
    rng = np.random.default_rng(3000 + n)
    v = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    sparse = np.where(rng.random(n) < 0.01, rng.integers(1, 1 << 32, n), 0).astype(np.uint32)
    edges = np.zeros(n, dtype=np.uint32)
    for k, i in enumerate((pu.SCO_EPB - 1, pu.SCO_EPB, pu.SCO_ROUND)):
        if i < n:
            edges[i] = k + 1
    for f in (sparse, edges, np.zeros(n, dtype=np.uint32)):
        wv, ws = pu.ref_seg_sum(v, f, True)
        check_scan(st, pu.SEG_SUM, pu.seg_pack(v, f), pu.seg_pack(wv, ws), inclusive=True)


def test_scratch_formula(st):
    """sco_scratch_elems: one fold per block and the total (the guard zone behind exactly that many elements is what the
    scan tests above watch)"""
    for n in SCAN_SIZES:
        assert pu.lib().pgrc_selftest_scratch_elems(n) == (n + pu.SCO_EPB - 1) // pu.SCO_EPB + 1


# ------------------------------------------------------------------------------------------------ the block scan
def block_input(kind, threads):
    rng = np.random.default_rng(5000 + 16 * threads + kind)
    if kind == pu.BLK_SEG:
        f = np.where(rng.random(threads) < 0.03, rng.integers(1, 1 << 32, threads), 0).astype(np.uint32)
        if threads >= 128:
            f[63], f[64] = 5, 6                             # flags on both sides of a wave edge
        return pu.seg_pack(rng.integers(-(1 << 40), 1 << 40, threads), f)
    width = 32 if kind == pu.BLK_SUM_U32 else 64
    return rng.integers(0, 1 << width, threads, dtype=np.uint64).astype(pu.BLOCK_TYPES[kind])


@pytest.mark.parametrize("threads", [64, 128, 256, 512, 1024])
@pytest.mark.parametrize("kind", [pu.BLK_SUM_U32, pu.BLK_SUM_U64, pu.BLK_MAX_U64, pu.BLK_SEG], ids=["sum32", "sum64", "max64", "seg"])
def test_block_scan(st, kind, threads):
    """sco_block_exclusive with the wave count static and from blockDim.x, SYNC_AFTER both ways: every thread's exclusive value,
    the same correct total in every thread, and a second scan in the same kernel over the same smem"""
    x = block_input(kind, threads)
    ex, tot, second = pu.ref_block(kind, x)
    for nwv_static in (True, False):
        for sync_after in (True, False):
            gex, gtot, gsec, guards = st.block_scan(kind, x, nwv_static, sync_after)
            what = f"threads {threads} static {nwv_static} sync_after {sync_after}"
            assert guards == 7, f"{what}: guard zones written: {guards:#x}"
            assert np.array_equal(gex, ex), f"{what}: exclusive values differ at threads {np.flatnonzero(gex != ex)[:8]}"
            assert np.all(gtot == gtot[0]), f"{what}: the threads were handed different totals"
            assert gtot[0] == tot, f"{what}: total {gtot[0]}, want {tot}"
            assert np.array_equal(gsec, second), f"{what}: the second scan differs at threads {np.flatnonzero(gsec != second)[:8]}"


# ------------------------------------------------------------------------------------------------ the stable sort
SORT_SIZES = [0, 1, 2, 63, 64, 65, 8191, 8192, 8193, 16384, 16385, 1000003]
SORT_FIELDS = [(0, 1), (0, 8), (0, 9), (3, 24), (0, 31), (0, 33), (5, 38), (32, 64), (0, 64), (7, 7)]
KEY_SETS = ["uniform", "all-equal", "two-values", "descending", "one-digit-wave", "index-mod-256"]


def field_values(name, n, w, rng):
    """n field values below 2^w"""
    top = 1 << w
    i = np.arange(n, dtype=np.uint64)
    if name == "uniform":
        return rng.integers(0, top, n, dtype=np.uint64)
    if name == "all-equal":                                 # one digit per tile: per-wave counts of 512, a run of 8192
        return np.full(n, rng.integers(0, top, dtype=np.uint64), dtype=np.uint64)
    if name == "two-values":
        a = int(rng.integers(0, top, dtype=np.uint64))
        return np.array([a, a ^ (1 | top >> 1)], dtype=np.uint64)[rng.integers(0, 2, n)]      # they differ in the lowest and in the highest digit
    if name == "descending":
        rev = np.uint64(max(n - 1, 0)) - i
        return rev * np.uint64(min(top // n, M64)) if top >= n > 0 else (rev >> np.uint64(max(int(n - 1).bit_length() - w, 0))) & np.uint64(top - 1)
    if name == "one-digit-wave":                            # every second run of 512 records shares one value, the others count up
        return np.where((i // np.uint64(512)) % np.uint64(2) == 1, rng.integers(0, top, dtype=np.uint64), i & np.uint64(top - 1))
    if name == "index-mod-256":
        return (i % np.uint64(256)) & np.uint64(top - 1)
    raise KeyError(name)


def make_keys(name, n, bit_lo, bit_hi, seed):
    """field values by `name`, random bits everywhere else"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    w = bit_hi - bit_lo
    if w <= 0:
        return keys
    fmask = ((1 << w) - 1) << bit_lo
    return (keys & np.uint64(M64 ^ fmask)) | (field_values(name, n, w, rng) << np.uint64(bit_lo))


@pytest.mark.parametrize("bit_lo,bit_hi", SORT_FIELDS)
@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_is_stable_by_the_field(st, n, bit_lo, bit_hi):
    """keys only and pairs: the output is the input in the order of a stable sort by the field -- whole records, random bits
    outside the field included, and the input index as the value, so equal fields in any other order fail; (7, 7) sorts nothing"""
    for k, name in enumerate(KEY_SETS):
        keys = make_keys(name, n, bit_lo, bit_hi, 7000 + 31 * n + 7 * bit_lo + bit_hi + 1000 * k)
        if n >= 8192 and bit_hi - bit_lo >= 8 and name == "all-equal":
            assert np.unique(pu.field_of(keys, bit_lo, bit_hi)).size == 1
        order = pu.ref_stable_order(keys, bit_lo, bit_hi) if bit_hi > bit_lo else np.arange(n)
        want = keys[order]
        what = f"{name} n {n} bits [{bit_lo}, {bit_hi})"
        gk, _, guards = st.sort(keys, None, bit_lo, bit_hi)
        assert guards == 15, f"{what}, keys only: guard zones written: {guards:#x}"
        assert np.array_equal(gk, want), f"{what}, keys only: first difference at {np.flatnonzero(gk != want)[:4]}"
        gk, gv, guards = st.sort(keys, np.arange(n, dtype=np.uint64), bit_lo, bit_hi)
        assert guards == 15, f"{what}, pairs: guard zones written: {guards:#x}"
        assert np.array_equal(gk, want), f"{what}, pairs: keys differ first at {np.flatnonzero(gk != want)[:4]}"
        assert np.array_equal(gv, order.astype(np.uint64)), f"{what}, pairs: not the stable order, first at {np.flatnonzero(gv != order)[:4]}"


# ------------------------------------------------------------------------------------------------ the segment sort
SEG_SIZES = [0, 1, 2, 3] * 4 + [64, 65] * 2 + [4600, 8191, 8192, 8193, 8193, 20000]


@functools.lru_cache(maxsize=1)
def segment_bounds():
    sizes = np.array(SEG_SIZES)[np.random.default_rng(81).permutation(len(SEG_SIZES))]
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    seg.setflags(write=False)
    return seg


@pytest.mark.parametrize("cap", [8, 1])
@pytest.mark.parametrize("top_bits", [32, 8])
@pytest.mark.parametrize("keyset", ["uniform", "equal-top-32"])
@pytest.mark.parametrize("bit_lo,bit_hi", [(0, 24), (8, 48), (16, 64)])
def test_segment_sort(st, bit_lo, bit_hi, keyset, top_bits, cap):
    """every segment of at most 8192 pairs comes back sorted by the field with its own pairs; larger ones come back untouched,
    counted in ovl[0] and listed up to cap.  top_bits = 8 makes the short way fail at every width; at top_bits = 32 the keys that
    agree in the field's top 32 bits make it fail for the 40- and 48-bit fields (a field of at most top_bits bits is sorted whole
    by the short way, so the 24-bit field reaches the long way through top_bits = 8 alone).  (Pairs with equal fields may come in
    any order: radix.hip promises none there.)"""
    seg = segment_bounds()
    n, w = int(seg[-1]), bit_hi - bit_lo
    rng = np.random.default_rng(9000 + 64 * bit_lo + bit_hi + (1 if keyset == "uniform" else 2))
    keys = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if keyset == "equal-top-32":                           # per segment one value in the field's top 32 bits (all of a 24-bit field but its low byte)
        low = max(w - 32, 8)
        segno = np.repeat(np.arange(seg.size - 1), np.diff(seg.astype(np.int64)))
        tops = rng.integers(0, 1 << (w - low), seg.size - 1, dtype=np.uint64)[segno]
        f = (tops << np.uint64(low)) | rng.integers(0, 1 << low, n, dtype=np.uint64)
        fmask = ((1 << w) - 1) << bit_lo
        keys = (keys & np.uint64(M64 ^ fmask)) | (f << np.uint64(bit_lo))
    vals = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    gk, gv, ovl, guards = st.sort_segments(keys, vals, seg, bit_lo, bit_hi, top_bits, cap)
    assert guards == 7, f"guard zones written (keys, values, overflow list): {guards:#x}"
    big = [s for s in range(seg.size - 1) if int(seg[s + 1]) - int(seg[s]) > pu.RX_TILE]
    assert len(big) == 3
    for s in range(seg.size - 1):
        a, b = int(seg[s]), int(seg[s + 1])
        if s in big:
            assert np.array_equal(gk[a:b], keys[a:b]) and np.array_equal(gv[a:b], vals[a:b]), f"segment {s} of {b - a} pairs was touched"
            continue
        f = pu.field_of(gk[a:b], bit_lo, bit_hi)
        assert np.all(f[1:] >= f[:-1]), f"segment {s} of {b - a} pairs does not ascend in the field"
        got = np.stack([gk[a:b], gv[a:b]], axis=1)
        want = np.stack([keys[a:b], vals[a:b]], axis=1)
        assert np.array_equal(got[np.lexsort((got[:, 1], got[:, 0]))], want[np.lexsort((want[:, 1], want[:, 0]))]), f"segment {s}: not the input's pairs"
    assert ovl[0] == len(big)
    listed = ovl[1:1 + min(len(big), cap)].tolist()
    assert len(set(listed)) == len(listed) and set(listed) <= set(big), f"overflow list {listed}, oversized segments {big}"
    assert np.array_equal(ovl[1 + len(listed):], pu.fill_of(np.uint32, cap - len(listed))), "the overflow list was written past the count"
