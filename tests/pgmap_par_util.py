"""The parallel form of markAndRemoveExactMatches, vectorised in numpy: what pgmap.hip computes, step by
step and without a loop over the matches, so that every step can be held to the literal loop of pgmap_util.mark_and_remove
on the CPU.

  normalise     the strand correction and the same-text collision rule per match
  order         sort by (dst, src, len), drop equal triples, drop matches shorter than min_len
  threshold     with the running position p, match i is kept iff p <= t_i = e_i - min_len, and then p = e_i
  next          next(i) = the first j > i with t_j >= e_i.  A match i with an earlier k, t_k >= e_i, is never kept ("dead");
                for every other i it is the first j at all whose prefix maximum of t reaches e_i: one binary search
  path          the kept matches = the path from match 0 through next, marked by pointer jumping
  marks         d' = max(dst, e of the kept predecessor), s' = src (+ d' - dst on the forward strand), L' = e - d'
  streams       offsets at fixed width, byte-frugal lengths laid out by a scan of their widths
  text          a scan of L' places every mark in the mapped text; every mapped byte finds its literal run by binary search"""
from __future__ import annotations

import numpy as np

import pgmap_util as pu


def normalise(matches, n2: int, dest_is_src: bool, rev_compl: bool):
    m = np.asarray(matches, dtype=np.uint64).reshape(-1, 3)
    src, ln, dst = (m[:, 0].astype(np.int64), m[:, 1].astype(np.int64), m[:, 2].astype(np.int64))
    if rev_compl:
        dst = n2 - (dst + ln)
    if dest_is_src:
        src, dst = np.minimum(src, dst), np.maximum(src, dst)
        if rev_compl:
            margin = np.where(src + ln > dst, (src + ln - dst + 1) // 2, 0)
            ln, dst = ln - margin, dst + margin
    return dst, src, ln


def ordered_unique(dst, src, ln, min_len: int):
    """-> (dst, src, e) of the matches that enter the greedy pass, in TextMatch's order; the count of different triples"""
    order = np.lexsort((ln, src, dst))
    dst, src, ln = dst[order], src[order], ln[order]
    first = np.ones(dst.size, dtype=bool)
    first[1:] = (dst[1:] != dst[:-1]) | (src[1:] != src[:-1]) | (ln[1:] != ln[:-1])
    alive = first & (ln >= min_len)
    return dst[alive], src[alive], (dst + ln)[alive], int(first.sum())


def next_pointers(e, min_len: int):
    """next(i) by the prefix maximum of t (n = none), and the dead flags"""
    n = e.size
    t = e - min_len
    pmax = np.maximum.accumulate(t) if n else t
    dead = np.zeros(n, dtype=bool)
    dead[1:] = pmax[:-1] >= e[1:]
    nxt = np.searchsorted(pmax, e, side="left")
    nxt[dead] = n
    return nxt, dead, t


def path(nxt):
    """kept flags by pointer jumping from match 0, and the number of passes"""
    n = nxt.size
    kept = np.zeros(n + 1, dtype=bool)
    if n:
        kept[0] = True
    jump = np.append(nxt, n)
    passes, reach = 0, 1
    while reach < n:
        kept[jump[kept]] = True
        jump = jump[jump]
        reach <<= 1
        passes += 1
    return kept[:n], passes


def marks_of(dst, src, e, kept, rev_compl: bool):
    d, s, ee = dst[kept], src[kept], e[kept]
    p = np.concatenate([[0], ee[:-1]]).astype(np.int64)
    dp = np.maximum(d, p)
    sp = s if rev_compl else s + (dp - d)
    return dp, sp, ee - dp


def frugal_widths(v):
    v = np.asarray(v, dtype=np.uint64)
    w = np.ones(v.size, dtype=np.int64)
    x = v >> np.uint64(7)
    while x.any():
        w += x > 0
        x = x >> np.uint64(7)
    return w


def streams(sp, lp, min_len: int, src_len: int):
    width = 4 if src_len <= pu.UINT32_MAX else 8
    off = sp.astype("<u4" if width == 4 else "<u8").tobytes()
    v = (lp - min_len).astype(np.uint64)
    w = frugal_widths(v)
    hdr = pu.frugal_stream([min_len])
    at = len(hdr) + np.concatenate([[0], np.cumsum(w)]).astype(np.int64)
    out = np.zeros(int(at[-1]), dtype=np.uint8)
    out[:len(hdr)] = np.frombuffer(hdr, np.uint8)
    for b in range(10):                                   # byte b of every value that has one
        has = w > b
        byte = (v[has] >> np.uint64(7 * b)) & np.uint64(127)
        out[at[:-1][has] + b] = (byte + np.where(w[has] > b + 1, 128, 0).astype(np.uint64)).astype(np.uint8)
    return off, out.tobytes()


def mapped_text(dest, dp, lp):
    dest = np.ascontiguousarray(dest, dtype=np.uint8)
    k = np.arange(dp.size, dtype=np.int64)
    cum = np.concatenate([[0], np.cumsum(lp)]).astype(np.int64)
    mp = dp - cum[:-1] + k                                 # the marks' places in the mapped text
    mapped_len = dest.size - int(cum[-1]) + dp.size
    o = np.arange(mapped_len, dtype=np.int64)
    r = np.searchsorted(mp, o, side="left")               # marks before byte o
    is_mark = np.zeros(mapped_len, dtype=bool)
    is_mark[mp] = True
    x = np.minimum(o - r + cum[r], max(dest.size - 1, 0))
    out = np.where(is_mark, pu.MATCH_MARK, dest[x] if dest.size else 0).astype(np.uint8)
    return out.tobytes(), mp


def mark_and_remove_parallel(dest, matches, dest_is_src: bool, rev_compl: bool, min_len: int, src_len: int, detail: bool = False):
    dest = np.ascontiguousarray(dest, dtype=np.uint8)
    dst, src, ln = normalise(matches, dest.size, dest_is_src, rev_compl)
    dst, src, e, n_unique = ordered_unique(dst, src, ln, min_len)
    nxt, dead, t = next_pointers(e, min_len)
    kept, passes = path(nxt)
    dp, sp, lp = marks_of(dst, src, e, kept, rev_compl)
    off, lens = streams(sp, lp, min_len, src_len)
    mapped, mp = mapped_text(dest, dp, lp)
    if detail:
        return mapped, off, lens, {"dst": dst, "e": e, "t": t, "next": nxt, "dead": dead, "kept": kept, "passes": passes, "mp": mp,
                                   "unique": n_unique, "dp": dp, "sp": sp, "lp": lp}
    return mapped, off, lens


def greedy_kept(e, min_len: int):
    """the threshold rule, literally (the checker of next_pointers / path)"""
    kept = np.zeros(e.size, dtype=bool)
    p = 0
    for i, ei in enumerate(e.tolist()):
        if p <= ei - min_len:
            kept[i] = True
            p = ei
    return kept


def random_case(rng, n2: int, src_len: int, count: int, min_len: int, dest_is_src: bool, rev_compl: bool):
    """a hand-made match list with the features no fixture has: duplicates, piles inside one long match, chains of overlapping
    matches, matches that fall below min_len after the collision margin, src == dst, a mark at 0, a mark that ends at n2 and
    adjacent marks.  Not real matches: the mapping does not look at symbols."""
    if dest_is_src:
        src_len = n2
    rows = []

    def add(s, ln, d):
        ln = int(min(ln, src_len - s, n2 - d))
        if ln > 0 and 0 <= s and 0 <= d:
            rows.append((s, ln, d))

    for _ in range(count):
        ln = int(rng.integers(1, 4 * min_len))
        add(int(rng.integers(0, src_len)), ln, int(rng.integers(0, n2)))
    if rows:
        for _ in range(count // 4 + 1):                                   # duplicates
            rows.append(rows[int(rng.integers(0, len(rows)))])
    big = int(rng.integers(0, max(1, n2 // 2)))                           # a long match with a pile inside, then a chain
    blen = min(n2 - big, src_len, 12 * min_len)
    add(0, blen, big)
    for _ in range(count // 3):
        add(int(rng.integers(0, src_len)), int(rng.integers(min_len, 3 * min_len)), big + int(rng.integers(0, max(1, blen))))
    at = big + blen
    for _ in range(count // 3):
        add(int(rng.integers(0, src_len)), min_len + int(rng.integers(0, min_len)), at)
        at += int(rng.integers(1, min_len + 2))
    L = min(min_len + 3, n2, src_len)
    add(5 % max(1, src_len - L + 1), L, 0)                                # at matchTexts' position 0 and at its end: with
    add(0, L, n2 - L)                                                     # rev_compl the mark that ends at n2 / starts at 0
    if n2 >= 4 * L and src_len >= L:
        q = n2 // 2
        add(1 % max(1, src_len - L + 1), L, q)                            # adjacent marks: "%%"
        add(2 % max(1, src_len - L + 1), L, q + L)
    if dest_is_src:
        add(0, L, 0)                                                      # (the only mark at 0 a text mapped onto itself can have)
        s = int(rng.integers(0, max(1, n2 - 2 * min_len)))
        add(s, 2 * min_len, n2 - s - 2 * min_len if rev_compl else s)      # src == dst after normalisation
        add(s, min_len + 1, min(n2 - min_len - 1, max(0, n2 - s - min_len - 1 - (min_len // 2))) if rev_compl else s + 1)   # below min_len after the margin
    m = np.asarray(rows, dtype=np.uint64).reshape(-1, 3)
    return m[rng.permutation(m.shape[0])]
