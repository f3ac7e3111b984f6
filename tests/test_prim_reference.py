"""The numpy references of tests/prim_util.py against a literal loop of each operator (no GPU): what
tests/test_gpu_primitives.py holds the kernels to must itself be right."""
import numpy as np
import pytest

import prim_util as pu

M64 = (1 << 64) - 1


def fold(op, ident, xs, inclusive):
    """the scan as scanops.h defines it: out(i) = the fold of ident, x[0], ..., x[i] (inclusive) or ..., x[i-1]"""
    out, acc = [], ident
    for x in xs:
        nxt = op(acc, x)
        out.append(nxt if inclusive else acc)
        acc = nxt
    return out, acc


def last_valid_inputs():
    rng = np.random.default_rng(11)
    n = 300
    some = np.where(rng.random(n) < 0.1, rng.integers(0, 1000, n), pu.NONE).astype(np.uint32)
    none = np.full(n, pu.NONE, dtype=np.uint32)
    first = none.copy()
    first[0] = 7
    lastonly = none.copy()
    lastonly[-1] = 9
    dense = rng.integers(0, 50, n).astype(np.uint32)
    return {"some": some, "all-identity": none, "first-only": first, "last-only": lastonly, "dense": dense, "one": np.array([5], dtype=np.uint32),
            "empty": np.zeros(0, dtype=np.uint32)}


@pytest.mark.parametrize("name", list(last_valid_inputs()))
@pytest.mark.parametrize("inclusive", [False, True])
def test_last_valid_is_the_fold_of_its_operator(name, inclusive):
    x = last_valid_inputs()[name]
    want, _ = fold(lambda a, b: b if b != pu.NONE else a, pu.NONE, [int(v) for v in x], inclusive)
    assert pu.ref_last_valid(x, inclusive).tolist() == want


def seg_inputs():
    rng = np.random.default_rng(12)
    n = 400
    v = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    some = np.where(rng.random(n) < 0.05, rng.integers(1, 4, n), 0).astype(np.uint32)
    edge = np.zeros(n, dtype=np.uint32)
    edge[[0, 63, 64, 255, 256, n - 1]] = [1, 2, 1, 3, 1, 2]         # flags at the first and last element and at wave and block edges
    big = v.copy()
    big[:3] = [(1 << 63) - 1, (1 << 63) - 1, 5]                     # the sum wraps in 64 bits, as the kernel's does
    return {"some": (v, some), "no-flag": (v, np.zeros(n, dtype=np.uint32)), "edge": (v, edge), "all-flags": (v, np.ones(n, dtype=np.uint32)),
            "wraps": (big, some), "empty": (v[:0], some[:0])}


def seg_loop_op(a, b):
    if b[1]:
        return b
    s = (a[0] + b[0]) & M64
    return (s - (1 << 64) if s >> 63 else s, a[1])


@pytest.mark.parametrize("name", list(seg_inputs()))
@pytest.mark.parametrize("inclusive", [False, True])
def test_segmented_sum_is_the_fold_of_its_operator(name, inclusive):
    v, f = seg_inputs()[name]
    want, _ = fold(seg_loop_op, (0, 0), list(zip(v.tolist(), f.tolist())), inclusive)
    gv, gs = pu.ref_seg_sum(v, f, inclusive)
    assert list(zip(gv.tolist(), gs.tolist())) == want
    a, b = pu.seg_pack(v, f), pu.seg_pack(v[::-1], f[::-1])
    got = pu.seg_op(a, b)
    assert list(zip(got["v"].tolist(), got["set"].tolist())) == [seg_loop_op(x, y) for x, y in zip(zip(v.tolist(), f.tolist()), zip(v[::-1].tolist(), f[::-1].tolist()))]


@pytest.mark.parametrize("width,start", [(32, 0), (64, 0), (64, (1 << 40) + 12345)])
@pytest.mark.parametrize("inclusive", [False, True])
def test_wrapped_sum_is_the_fold_of_its_operator(width, start, inclusive):
    rng = np.random.default_rng(13)
    x = rng.integers(0, 1 << width, 300, dtype=np.uint64)
    mask = (1 << width) - 1
    want, total = fold(lambda a, b: (a + b) & mask, start & mask, [int(v) for v in x], inclusive)
    got, gt = pu.ref_sum(x, width, start, inclusive)
    assert got.tolist() == want and int(gt) == total
    got, gt = pu.ref_sum(x[:0], width, start, inclusive)
    assert got.size == 0 and int(gt) == start & mask


@pytest.mark.parametrize("inclusive", [False, True])
def test_maximum_is_the_fold_of_its_operator(inclusive):
    x = np.random.default_rng(14).integers(0, 1 << 64, 300, dtype=np.uint64)
    want, _ = fold(max, 0, [int(v) for v in x], inclusive)
    assert pu.ref_max(x, inclusive).tolist() == want


@pytest.mark.parametrize("kind", [pu.BLK_SUM_U32, pu.BLK_SUM_U64, pu.BLK_MAX_U64, pu.BLK_SEG])
def test_block_reference_is_two_folds(kind):
    """exclusive scan, total, and the exclusive scan of op(first exclusive value, the input reversed)"""
    rng = np.random.default_rng(15)
    n = 128
    if kind == pu.BLK_SEG:
        v, f = rng.integers(-1000, 1000, n), np.where(rng.random(n) < 0.1, 1, 0)
        x = pu.seg_pack(v, f)
        xs, op, ident = list(zip(v.tolist(), f.tolist())), seg_loop_op, (0, 0)
        un = lambda a: list(zip(a["v"].tolist(), a["set"].tolist()))        # noqa: E731
    else:
        width = 32 if kind == pu.BLK_SUM_U32 else 64
        x = rng.integers(0, 1 << width, n, dtype=np.uint64).astype(pu.BLOCK_TYPES[kind])
        xs, ident = [int(t) for t in x], 0
        op = max if kind == pu.BLK_MAX_U64 else (lambda a, b: (a + b) & ((1 << width) - 1))
        un = lambda a: [int(t) for t in a]                                   # noqa: E731
    ex, tot = fold(op, ident, xs, False)
    second, _ = fold(op, ident, [op(e, r) for e, r in zip(ex, xs[::-1])], False)
    gex, gtot, gsec = pu.ref_block(kind, x)
    assert un(gex) == ex and un(np.array([gtot], dtype=x.dtype)) == [tot] and un(gsec) == second


@pytest.mark.parametrize("bit_lo,bit_hi", [(0, 1), (0, 8), (3, 24), (5, 38), (32, 64), (0, 64), (7, 7)])
def test_stable_field_order_is_an_insertion_sort(bit_lo, bit_hi):
    rng = np.random.default_rng(16)
    n = 300
    keys = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if bit_hi - bit_lo > 3:                                # many equal fields, so that stability shows
        fmask = ((1 << (bit_hi - bit_lo)) - 1) << bit_lo
        keys = (keys & np.uint64(M64 ^ fmask)) | (rng.integers(0, 8, n, dtype=np.uint64) << np.uint64(bit_hi - 3))
    w = bit_hi - bit_lo
    order = []
    for i, k in enumerate(int(k) for k in keys):           # insert behind every record whose field is not larger
        f = (k >> bit_lo) & ((1 << w) - 1)
        j = len(order)
        while j > 0 and order[j - 1][0] > f:
            j -= 1
        order.insert(j, (f, i))
    assert pu.ref_stable_order(keys, bit_lo, bit_hi).tolist() == [i for _, i in order]
    assert pu.field_of(keys, bit_lo, bit_hi).tolist() == [(int(k) >> bit_lo) & ((1 << w) - 1) for k in keys]


def test_digit_split_of_every_field_width():
    """rx_sort's passes: ceil(bits / 8) of them, digits of at most 8 bits that sum to the field and differ by at most one"""
    for bits in range(1, 65):
        d = pu.rx_split(bits)
        assert len(d) == (bits + 7) // 8 and sum(d) == bits and max(d) <= 8 and min(d) >= 1 and max(d) - min(d) <= 1, (bits, d)
        assert d == sorted(d, reverse=True)
    assert pu.rx_split(31) == [8, 8, 8, 7] and pu.rx_split(33) == [7, 7, 7, 6, 6] and pu.rx_split(64) == [8] * 8 and pu.rx_split(1) == [1]
