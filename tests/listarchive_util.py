"""The archive form of a reads list's mismatch streams (include/pgrc_decode.h, "The archive form"), restated
twice on the CPU.

LITERAL: the loops of SeparatedPseudoGenomeOutputBuilder::toStringAndSeparateZeros
(pseudogenome/persistence/SeparatedPseudoGenomePersistence.cpp:801-813), reorderingSymbolsExclusiveMismatchEncoding
(:1115-1138) and compressRlMisRevOffDest (:823-903), and of the reassembly in ExtendedReadsListWithConstantAccessOption::
loadConstantAccessExtendedReadsList (pseudogenome/readslist/SeparatedExtendedReadsList.cpp:253-285), value by value.  (The one
liberty: compressRlMisRevOffDest moves an entry's offsets to their destination as one slice, not byte by byte.)

PARALLEL: what the device does -- flags and cumulative sums, a bincount, and stable per-count ranks from
np.argsort(kind="stable").

Streams are a dict: n_entries, n_mismatches, n_nonzero, zero_flags, nonzero_cnt, mis_sym, bases_order (5 bytes), props,
dests (a list, dests[c] = destination c, [0] empty).  A loaded list is (mis_cnt, mis_sym codes, forward offsets)."""
import glob
import os

import numpy as np

ACGTN = b"ACGTN"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U8 = np.uint8


def _u8(a):
    return np.ascontiguousarray(a, dtype=U8).reshape(-1)


# ---------------------------------------------------------------- literal encoder
def separate_zeros_literal(mis_cnt):
    """toStringAndSeparateZeros -> (zero flags, the non-zero counts)"""
    tmp = bytearray(_u8(mis_cnt).tobytes())
    flags = bytearray()
    j = 0
    for i in range(len(tmp)):
        is_zero = tmp[i] == 0
        flags.append(is_zero)
        if not is_zero:
            tmp[j] = tmp[i]
            j += 1
    del tmp[j:]
    return np.frombuffer(bytes(flags), U8), np.frombuffer(bytes(tmp), U8)


def reorder_symbols_literal(mis_sym):
    """reorderingSymbolsExclusiveMismatchEncoding -> (codes, bases order); std::sort on five elements is libstdc++'s insertion
    sort: an element moves left past every element the comparison puts it before, so equal counts keep A C G T N"""
    src = _u8(mis_sym).tobytes()
    counts = [0] * 5
    for c in src:
        counts[c & 15] += 1
    order = [0, 1, 2, 3, 4]
    for i in range(1, 5):
        v, j = order[i], i
        while j > 0 and counts[v] > counts[order[j - 1]]:
            order[j] = order[j - 1]
            j -= 1
        order[j] = v
    rev = [0] * 5
    for i in range(5):
        rev[order[i]] = i
    out = bytearray(len(src))
    for i, c in enumerate(src):
        actual, mismatch = rev[c >> 4], rev[c & 15]
        out[i] = mismatch - (1 if mismatch > actual else 0)
    return np.frombuffer(bytes(out), U8), bytes(ACGTN[v] for v in order)


def split_offsets_literal(mis_cnt, mis_rev_off, fast):
    """compressRlMisRevOffDest with separateFirstOffsetMode and transposeMode off -> (props, dests)"""
    off = _u8(mis_rev_off).tobytes()
    if fast:
        return np.array([1], U8), [np.zeros(0, U8), np.frombuffer(off, U8)]
    dests_count = 254
    cnt2dest = [dests_count] * 255
    for m in range(1, dests_count):
        cnt2dest[m] = m
    dests = [bytearray() for _ in range(255)]
    p = 0
    for c in _u8(mis_cnt).tobytes():
        if c:
            dests[cnt2dest[c]] += off[p:p + c]          # (c == 255 raises IndexError: the reference reads past its map)
            p += c
    while dests_count > 0 and len(dests[dests_count]) == 0:
        dests_count -= 1
    props = [dests_count] + [cnt2dest[m] for m in range(1, dests_count)]
    return np.array(props, U8), [np.frombuffer(bytes(d), U8) for d in dests[:dests_count + 1]]


def encode_literal(mis_cnt, mis_sym, mis_rev_off, fast=False):
    flags, nonzero = separate_zeros_literal(mis_cnt)
    codes, order = reorder_symbols_literal(mis_sym)
    props, dests = split_offsets_literal(mis_cnt, mis_rev_off, fast)
    return {"n_entries": flags.size, "n_mismatches": codes.size, "n_nonzero": nonzero.size, "zero_flags": flags, "nonzero_cnt": nonzero,
            "mis_sym": codes, "bases_order": order, "props": props, "dests": dests}


# ---------------------------------------------------------------- literal loader
def load_literal(st, L):
    """the loader's reassembly (:253-285) -> (misCnt, misSymCode, forward misOff)"""
    flags, nonzero = _u8(st["zero_flags"]).tobytes(), _u8(st["nonzero_cnt"]).tobytes()
    cnt = bytearray(len(flags))
    j = 0
    for i in range(len(flags)):
        if flags[i]:
            cnt[i] = 0
        else:
            cnt[i] = nonzero[j]
            j += 1
    props = _u8(st["props"]).tobytes()
    limit = props[0]
    cnt2src = [limit] * 255
    for m in range(1, limit):
        cnt2src[m] = props[m]
    srcs = [_u8(d).tobytes() for d in st["dests"]] + [b""] * 255
    counter = [0] * 255
    mis_off = bytearray()
    for i in range(len(cnt)):
        c = cnt[i]
        src = cnt2src[c] if c else 0
        start = len(mis_off)
        for _ in range(c):
            mis_off.append(srcs[src][counter[src]])
            counter[src] += 1
        # convertMisRevOffsets2Offsets (utils/helper.h:52-63)
        pos = L
        fwd = []
        for k in range(c):
            pos -= mis_off[start + k] + 1
            fwd.append(pos)
        mis_off[start:] = bytes(reversed(fwd))         # (a step below 0 raises: the reference's uint8 would wrap)
    return np.frombuffer(bytes(cnt), U8), _u8(st["mis_sym"]).copy(), np.frombuffer(bytes(mis_off), U8)


# ---------------------------------------------------------------- parallel forms
def stable_ranks(cnt):
    """-> (order, rank): the entries with a non-zero count, stably by count, and every such entry's rank among its count"""
    cnt = np.asarray(cnt, dtype=np.int64)
    nz = np.flatnonzero(cnt)
    order = nz[np.argsort(cnt[nz], kind="stable")]
    totals = np.bincount(cnt, minlength=256)
    first = np.concatenate([[0], np.cumsum(totals[1:])])[:-1]          # rank of the first entry of count c (c = 1 ..)
    rank = np.arange(order.size) - first[cnt[order] - 1]
    return order, rank, totals


def _byte_index(cnt, order, rank, totals):
    """for the mismatches in STREAM order: (where each lies in the stream, where in the joined destinations)"""
    cnt = np.asarray(cnt, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(cnt)])
    dstart = np.concatenate([[0], np.cumsum(np.arange(256) * totals)])[:256]
    c = cnt[order]
    k = np.arange(c.sum()) - np.repeat(np.concatenate([[0], np.cumsum(c)])[:-1], c)
    return np.repeat(starts[order], c) + k, np.repeat(dstart[c] + c * rank, c) + k, dstart


def encode_parallel(mis_cnt, mis_sym, mis_rev_off, fast=False):
    cnt, sym, off = _u8(mis_cnt), _u8(mis_sym), _u8(mis_rev_off)
    counts = np.bincount(sym & 15, minlength=5)[:5]
    order5 = sorted(range(5), key=lambda v: -counts[v])
    rev = np.zeros(16, dtype=np.int64)
    rev[order5] = np.arange(5)
    av, mv = rev[sym >> 4], rev[sym & 15]
    out = {"n_entries": cnt.size, "n_mismatches": sym.size, "n_nonzero": int((cnt != 0).sum()), "zero_flags": (cnt == 0).astype(U8),
           "nonzero_cnt": cnt[cnt != 0], "mis_sym": (mv - (mv > av)).astype(U8), "bases_order": bytes(ACGTN[v] for v in order5)}
    if fast:
        out["props"], out["dests"] = np.array([1], U8), [np.zeros(0, U8), off.copy()]
        return out
    assert not (cnt == 255).any()
    order, rank, totals = stable_ranks(cnt)
    src, dst, dstart = _byte_index(cnt, order, rank, totals)
    joined = np.empty(off.size, U8)
    joined[dst] = off[src]
    limit = int(np.flatnonzero(totals[1:]).max()) + 1 if off.size else 0
    out["props"] = np.array([limit] + list(range(1, limit)), U8)
    out["dests"] = [np.zeros(0, U8)] + [joined[dstart[c]:dstart[c] + c * totals[c]] for c in range(1, limit + 1)]
    return out


def load_parallel(st, L):
    flags = _u8(st["zero_flags"])
    cnt = np.zeros(flags.size, U8)
    cnt[flags == 0] = _u8(st["nonzero_cnt"])
    limit = int(_u8(st["props"])[0])
    m = int(cnt.sum(dtype=np.int64))
    if limit <= 1:
        rev_off = _u8(st["dests"][1]) if limit else np.zeros(0, U8)
    else:
        order, rank, totals = stable_ranks(cnt)
        src, dst, _ = _byte_index(cnt, order, rank, totals)
        joined = np.concatenate([_u8(d) for d in st["dests"][1:limit + 1]])
        rev_off = np.empty(m, U8)
        rev_off[src] = joined[dst]
    c64 = cnt.astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(c64)])[:-1]
    eid = np.repeat(np.arange(cnt.size), c64)
    k = np.arange(m) - starts[eid]
    cs = np.cumsum(rev_off.astype(np.int64) + 1)
    fwd = L - (cs - np.concatenate([[0], cs])[starts[eid]])
    out = np.empty(m, dtype=np.int64)
    out[starts[eid] + c64[eid] - 1 - k] = fwd
    return cnt, _u8(st["mis_sym"]).copy(), out.astype(U8)


# ---------------------------------------------------------------- generator
def make_list(seed, n, L, zero=0.7, counts=(1, 2, 3, 4, 5, 6), weights=None, skew=(5, 3, 8, 2, 1), same=0.0):
    """a list of n entries: mis_cnt (zero with probability `zero`, else one of `counts` by `weights`), context codes with the
    mismatch values drawn by `skew` (A C G T N) and the actual value another one (the same one with probability `same`), and
    rev-coded offsets that stay inside a read of L symbols -> (mis_cnt, mis_sym, mis_rev_off)"""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.min() >= 1 and counts.max() <= min(L, 255)
    w = np.ones(counts.size) if weights is None else np.asarray(weights, dtype=np.float64)
    cnt = counts[rng.choice(counts.size, size=n, p=w / w.sum())]
    cnt[rng.random(n) < zero] = 0
    m = int(cnt.sum())
    p = np.asarray(skew, dtype=np.float64)
    mv = rng.choice(5, size=m, p=p / p.sum())
    av = (mv + 1 + rng.integers(0, 4, size=m)) % 5
    av = np.where(rng.random(m) < same, mv, av)
    room = np.repeat(L // np.maximum(cnt, 1), cnt)                     # every r + 1 <= L / c: the c steps stay inside the read
    rev_off = (rng.random(m) * room).astype(np.int64)
    return cnt.astype(U8), ((av << 4) + mv).astype(U8), rev_off.astype(U8)


def rev_offsets(mis_cnt, fwd_off, L):
    """writeReadEntry's coding of ascending forward offsets (:975-981), vectorised"""
    cnt = np.asarray(mis_cnt, dtype=np.int64)
    off = np.asarray(fwd_off, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    eid = np.repeat(np.arange(cnt.size), cnt)
    k = np.arange(off.size) - starts[eid]
    nxt = np.where(k + 1 < cnt[eid], np.concatenate([off[1:], [0]]), L)     # the next offset of the entry, or L
    out = np.empty(off.size, dtype=np.int64)
    out[starts[eid] + cnt[eid] - 1 - k] = nxt - 1 - off
    return out.astype(U8)


def assert_streams(got, want):
    for k in ("n_entries", "n_mismatches", "n_nonzero"):
        assert int(got[k]) == int(want[k]), k
    assert bytes(got["bases_order"]) == bytes(want["bases_order"])
    for k in ("zero_flags", "nonzero_cnt", "mis_sym", "props"):
        assert _u8(got[k]).tobytes() == _u8(want[k]).tobytes(), k
    assert len(got["dests"]) == len(want["dests"])
    for c, (g, w) in enumerate(zip(got["dests"], want["dests"])):
        assert _u8(g).tobytes() == _u8(w).tobytes(), f"destination {c}"


# ---------------------------------------------------------------- fixtures
def fixtures():
    return sorted(glob.glob(os.path.join(GOLDEN, "listarchive_*.npz")))


def case_name(path):
    return os.path.basename(path)[len("listarchive_"):-len(".npz")]


def load_case(path):
    """-> (L, fast, inputs (mis_cnt, mis_sym, forward offsets, mis_rev_off), the reference's streams, its loaded list)"""
    z = np.load(path)
    limit = int(z["props"][0])
    st = {"n_entries": z["mis_cnt"].size, "n_mismatches": z["mis_sym"].size, "n_nonzero": z["nonzero_cnt"].size,
          "zero_flags": z["zero_flags"], "nonzero_cnt": z["nonzero_cnt"], "mis_sym": z["codes"], "bases_order": z["bases_order"].tobytes(),
          "props": z["props"], "dests": [np.zeros(0, U8)] + [z[f"dest{c}"] for c in range(1, limit + 1)]}
    inputs = (z["mis_cnt"], z["mis_sym"], z["mis_off"], rev_offsets(z["mis_cnt"], z["mis_off"], int(z["L"])))
    return int(z["L"]), bool(z["fast"]), inputs, st, (z["loaded_cnt"], z["loaded_sym"], z["loaded_off"])
