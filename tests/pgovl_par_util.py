"""Checker of the overlap search under the rule of the parallel generator (PGRC_OVL_RULE_PARALLEL), two things:

  literal          the reference's loops as they stand in ParallelGreedySwipingPackedOverlapPseudoGenomeGenerator.cpp with
                   avoidCyclesMode = false: prepareSortedReadsBlocks (:120-142, the order given), initAndFindDuplicates (:146-210),
                   mergeSortOfLeftSuffixes (:213-252) with updateSuffixQueue (:89-102), overlapSortedReadsAndSuffixes (:297-393),
                   blockPrefixOverlapSortedReadsAndSuffixesWithAfterSuffixMerge (:397-504) and the compare past the rows' end of
                   SymbolsPackingFacility::compareSequences(.., pos, length = 0).  Threads only share out blocks, so the loops
                   over threads are loops over blocks here
  parallel_form    the rule in the array form the device runs: the sweeps of pgovl_util.parallel_form with the weak order
                   reset at block starts and no drop rule; the merge in front of sweep L - 3 by prefix maxima of the follower
                   key; the regrouping of the last two sweeps as a concatenation.  Four switches turn it into the four
                   simplifications that are NOT the reference

Reads are numbered 1 .. R; the order among equal reads is an input, as in pgovl_util.  The follower key of read x is the
sequence of the dense ranks of the reads x + 1, x + 2, ...; a row past R is smaller than any row and a compare that meets one is
counted (`past_end_compares`): the reference reads memory behind its array there."""
import numpy as np

import pgovl_util as po
from pgovl_util import GROUPS, SYMBOL_ORDER, iterations

BLOCK_PREFIX = 3        # blockPrefixLength


def dense_read_ranks(codes, order):
    """rank[x] for x = 1 .. R: the number of distinct smaller reads; rank[0] unused, rank[R + 1] = -1 (no row)"""
    R, L = codes.shape
    order = np.asarray(order, dtype=np.int64)
    rows = np.ascontiguousarray(codes[order - 1] + 1).view("S%d" % L).ravel()
    new = np.concatenate([[0], (rows[1:] != rows[:-1]).astype(np.int64)])
    rank = np.full(R + 2, -1, dtype=np.int64)
    rank[order] = np.cumsum(new)
    return rank


class FollowerKey:
    """the compare of two reads by the rows that follow them; counts its calls"""

    def __init__(self, rank):
        self.rank = rank
        self.R = rank.size - 2
        self.compares = 0
        self.past_end = 0

    def cmp(self, x, y, count=True):
        assert x != y
        k = 1
        while True:
            a, b = x + k, y + k
            if a > self.R or b > self.R:
                res = -1 if a > b else 1            # the one whose rows end first is the smaller
                if count:
                    self.compares += 1
                    self.past_end += 1
                return res
            if self.rank[a] != self.rank[b]:
                if count:
                    self.compares += 1
                return -1 if self.rank[a] < self.rank[b] else 1
            k += 1


def tail_sweeps(L, coef):
    """sweeps of a run that pair whole blocks: i >= L - 3"""
    iters = iterations(L, coef)
    return sum(1 for i in range(1, iters) if i >= L - BLOCK_PREFIX)


# ------------------------------------------------------------------------------------------------ the literal loops
def literal(codes, order, coef, symbols):
    """-> as pgovl_util.literal, and `counters`: follower_compares, past_end_compares of the reference's own queue"""
    codes = np.asarray(codes, dtype=np.uint8)
    R, L = codes.shape
    assert L > BLOCK_PREFIX, "the reference reads symbol 3 of every read"
    sc = int(symbols)
    B = sc ** BLOCK_PREFIX
    rows = [codes[r].tobytes() for r in range(R)]
    fk = FollowerKey(dense_read_ranks(codes, order))

    def sym(r, off):
        return int(codes[r - 1, off])

    def cmp_suffixes(l, r, off):                        # comparePackedReads(l - 1, r - 1, off)
        if off >= L:
            return fk.cmp(l, r)
        a, b = rows[l - 1][off:], rows[r - 1][off:]
        return (a > b) - (a < b)

    def cmp_sp(s, p, off):
        a, b = rows[s - 1][off:], rows[p - 1][:L - off]
        return (a > b) - (a < b)

    nxt = np.zeros(R + 1, dtype=np.uint32)
    ov = np.zeros(R + 1, dtype=np.uint16)
    reads_left = R
    # prepareSortedReadsBlocks
    sr = [int(x) for x in order]
    blk = np.array([(sym(r, 0) * sc + sym(r, 1)) * sc + sym(r, 2) for r in sr], dtype=np.int64)
    rpos = [int(np.searchsorted(blk, b, side="left")) for b in range(B)] + [R]
    rcount = [0] * B
    plus = [[0] * (sc + 1) for _ in range(B + 1)]       # sortedSuffixBlockPlusSymbolPos
    spos = [0] * (B + 1)                                # sortedSuffixBlockPos

    # initAndFindDuplicates<false>
    left_count = [0] * B
    for b in range(B):
        rcount[b] = rpos[b + 1] - rpos[b]
        cur = 0
        plus[b][0] = rpos[b]
        young = (b % (B // sc)) * sc
        j = rpos[b]
        while j < rpos[b + 1]:
            j += 1
            if j < rpos[b + 1] and rows[sr[j - 1] - 1] == rows[sr[j] - 1]:
                nxt[sr[j - 1]] = sr[j]
                ov[sr[j - 1]] = L
                reads_left -= 1
            else:
                s = sym(sr[j - 1], BLOCK_PREFIX)
                left_count[young + s] += 1
                while cur != s:
                    cur += 1
                    plus[b][cur] = j - 1
        while cur < sc:
            cur += 1
            plus[b][cur] = rpos[b + 1]
    duplicates = R - reads_left

    def merge_sort_of_left(offset, counts, src):
        nonlocal spos
        spos = [0] * (B + 1)
        for b in range(1, B + 1):
            spos[b] = spos[b - 1] + counts[b - 1]
        dst = [0] * spos[B]
        for b in range(B):
            prev_young, last = b // sc, b % sc
            idx = [plus[prev_young + (B // sc) * j][last] for j in range(sc)]
            end = [plus[prev_young + (B // sc) * j][last + 1] for j in range(sc)]
            queue = []

            def update(g):
                if idx[g] < end[g]:
                    at = len(queue)
                    while True:
                        if at == 0 or cmp_suffixes(src[idx[g]], src[idx[queue[at - 1]]], offset + BLOCK_PREFIX) >= 0:
                            queue.insert(at, g)
                            break
                        at -= 1

            for j in range(sc):
                while idx[j] < end[j] and nxt[src[idx[j]]] != 0:
                    idx[j] += 1
                update(j)
            at = spos[b]
            while queue:
                j = queue.pop(0)
                dst[at] = src[idx[j]]
                at += 1
                idx[j] += 1
                while idx[j] < end[j] and nxt[src[idx[j]]] != 0:
                    idx[j] += 1
                update(j)
            assert at == spos[b + 1]
        return dst

    ss = merge_sort_of_left(1, left_count, sr)
    for b in range(B):                                  # the heads of the chains stay in the prefix list
        if not rcount[b]:
            continue
        i = rpos[b]
        for j in range(rpos[b], rpos[b] + rcount[b]):
            if j == 0 or nxt[sr[j - 1]] == 0:
                sr[i] = sr[j]
                i += 1
        rcount[b] = i - rpos[b]

    def pair_block(b, off, compare, on_left):
        """the walk of one block, shared by :319-389 and :402-459 (compare = False: every prefix of the block matches)"""
        nonlocal reads_left
        pre, pre_end = rpos[b], rpos[b] + rcount[b]
        suf, suf_end = spos[b], spos[b + 1]
        rcount[b] = 0
        while suf != suf_end or pre != pre_end:
            if suf == suf_end:
                sr[rpos[b] + rcount[b]] = sr[pre]
                rcount[b] += 1
                pre += 1
                continue
            s = ss[suf]
            res = -1
            start = pre
            while pre != pre_end:
                res = cmp_sp(s, sr[pre], off) if compare else 0
                if res != 0:
                    break
                if s != sr[pre]:
                    break
                res = -1
                pre += 1
            if res:
                pre = start
            else:
                p = sr[pre]
                while pre > start:
                    sr[pre] = sr[pre - 1]
                    pre -= 1
                sr[pre] = p
            if res == 0:
                nxt[s] = sr[pre]
                ov[s] = L - off
                reads_left -= 1
                pre += 1
            elif res > 0:
                sr[rpos[b] + rcount[b]] = sr[pre]
                rcount[b] += 1
                pre += 1
                continue
            else:
                on_left(s, suf)
            suf += 1

    log = [reads_left]
    iters = iterations(L, coef)
    cur_blocks = B
    for i in range(1, iters):
        if i < L - BLOCK_PREFIX:
            left_count = [0] * B
            for b in range(B):
                state = {"cur": 0}
                plus[b][0] = spos[b]
                young = (b % (B // sc)) * sc

                def on_left(s, suf, state=state, b=b, young=young):
                    c = sym(s, i + BLOCK_PREFIX)
                    left_count[young + c] += 1
                    while state["cur"] != c:
                        state["cur"] += 1
                        plus[b][state["cur"]] = suf

                pair_block(b, i, True, on_left)
                while state["cur"] < sc:
                    state["cur"] += 1
                    plus[b][state["cur"]] = spos[b + 1]
            ss = merge_sort_of_left(i + 1, left_count, ss)
        else:
            nb = cur_blocks // sc
            left_count = [0] * B
            for b in range(cur_blocks):
                def on_left(s, suf, b=b):
                    left_count[b % nb] += 1

                pair_block(b, i, False, on_left)
            if cur_blocks > sc:
                for b in range(nb):
                    root = b * sc
                    at = rpos[root] + rcount[root]
                    for b2 in range(1, sc):
                        for t in range(rpos[root + b2], rpos[root + b2] + rcount[root + b2]):
                            sr[at] = sr[t]
                            at += 1
                    rcount[root] = at - rpos[root]
                for b in range(1, nb):
                    rpos[b] = rpos[b * sc]
                    rcount[b] = rcount[b * sc]
                old = list(spos)
                spos2 = [0] * (B + 1)
                for b in range(1, nb + 1):
                    spos2[b] = spos2[b - 1] + left_count[b - 1]
                dst = []
                for b in range(nb):
                    for b2 in range(b, cur_blocks, nb):
                        dst += [x for x in ss[old[b2]:old[b2 + 1]] if nxt[x] == 0]
                    assert len(dst) == spos2[b + 1]
                for b in range(nb + 1):
                    spos[b] = spos2[b]
                ss = dst
            cur_blocks = nb
        log.append(reads_left)
    return {"next_read": nxt, "overlap": ov, "reads_left": np.array(log, dtype=np.uint64), "duplicates": duplicates,
            "links": R - reads_left - duplicates, "sweeps": max(iters - 1, 0),
            "counters": {"follower_compares": fk.compares, "past_end_compares": fk.past_end}}


# ------------------------------------------------------------------------------------------------ the array form
def quirk_places(S, g, gstart, vs, lens, lb, base, fk, cnt):
    """the merge in front of sweep L - 3: S in five groups (g, from gstart on), each in block order (vs = the block's dense
    value) and inside a block in the order it has.  A group's share of a block is cut into segments at the prefix maxima of the
    follower key; the block's segments come out by the key of their first element.  -> k, the place inside the block.
    Counted as the device counts: one compare of every element but a share's first with the maximum before it, and the compares
    of the searches a segment's first element makes in the other groups' shares"""
    n = S.size
    leader = np.zeros(n, dtype=np.int64)        # the place in S of the prefix maximum
    for j in range(n):
        first = j == gstart[g[j]] or vs[j - 1] != vs[j]
        if first:
            leader[j] = j
        else:
            m = leader[j - 1]
            leader[j] = j if fk.cmp(int(S[j]), int(S[m])) > 0 else m
    cnt["glued"] += int((leader != np.arange(n)).sum())
    k = np.zeros(n, dtype=np.int64)
    for j in range(n):
        m = int(leader[j])
        is_leader = m == j
        before = j - m
        for h in range(GROUPS):
            lo = int(gstart[h] + lb[vs[j], h])
            hi = lo + int(lens[vs[j], h])
            if h == g[j]:
                before += m - lo
                continue
            while lo < hi:                  # the first place of the share whose maximum is not below this one's
                mid = lo + ((hi - lo) >> 1)
                if fk.cmp(int(S[leader[mid]]), int(S[m]), count=is_leader) < 0:
                    lo = mid + 1
                else:
                    hi = mid
            before += lo - int(gstart[h] + lb[vs[j], h])
        k[j] = before
    return k


def parallel_form(codes, order, coef, symbols, reset=True, quirk=True, drop=False, concat=True):
    """as literal; `counters`: resets_changing (block starts at which the carried order of the groups was not the symbol
    order), follower_compares, past_end_compares, glued (suffixes whose key is below their group's prefix maximum),
    self_conflicts, would_drop (unpaired suffixes the serial rule would have removed).  reset=False, quirk=False, drop=True and
    concat=False are the four simplifications"""
    codes = np.asarray(codes, dtype=np.uint8)
    R, L = codes.shape
    assert L > BLOCK_PREFIX
    order = np.asarray(order, dtype=np.int64)
    nxt = np.zeros(R + 1, dtype=np.uint32)
    ov = np.zeros(R + 1, dtype=np.uint16)
    rows = np.ascontiguousarray(codes[order - 1] + 1).view("S%d" % L).ravel()
    same = rows[:-1] == rows[1:]
    nxt[order[:-1][same]] = order[1:][same]
    ov[order[:-1][same]] = L
    P = order[np.concatenate([[True], ~same])]
    S = order[np.concatenate([~same, [True]])]
    duplicates = int(same.sum())
    left = R - duplicates
    log = [left]
    fk = FollowerKey(dense_read_ranks(codes, order))
    cnt = dict(resets_changing=0, glued=0, self_conflicts=0, would_drop=0)
    iters = iterations(L, coef)
    for i in range(1, iters):
        if S.size == 0 or P.size == 0:
            log.append(left)
            continue
        m = L - i
        vs, vp = po.joint_ranks(codes, S, P, i)
        n = S.size
        g = codes[S - 1, i - 1].astype(np.int64)
        gstart = np.searchsorted(g, np.arange(GROUPS), side="left")
        nv = int(max(vs.max(), vp.max())) + 1
        lens = np.zeros((nv, GROUPS), dtype=np.int64)
        np.add.at(lens, (vs, g), 1)
        lb = np.cumsum(lens, axis=0) - lens
        base = np.cumsum(lens.sum(axis=1)) - lens.sum(axis=1)
        r = (np.arange(n) - gstart[g]) - lb[vs, g]
        ln = lens[vs]
        sym_k = np.minimum(ln, r[:, None]).sum(axis=1) + ((ln > r[:, None]) & (SYMBOL_ORDER[None, :] < g[:, None])).sum(axis=1)
        cat_k = (ln * (SYMBOL_ORDER[None, :] < g[:, None])).sum(axis=1) + r
        if i < L - BLOCK_PREFIX:
            runs = np.flatnonzero(lens.sum(axis=1) > 0)
            state = np.repeat(SYMBOL_ORDER[None, :], nv, axis=0)
            # the block of a run: the first three symbols of the suffix; runs are in suffix order, so blocks are contiguous
            first_of = np.zeros(nv, dtype=np.int64)
            first_of[vs] = S
            b3 = codes[first_of[runs] - 1, i:i + BLOCK_PREFIX].astype(np.int64)
            bid = (b3[:, 0] * GROUPS + b3[:, 1]) * GROUPS + b3[:, 2]
            starts = np.flatnonzero(np.concatenate([[True], bid[1:] != bid[:-1]]))
            carried = po.states_before(SYMBOL_ORDER, lens[runs])        # without any reset
            if reset:
                for a, z in zip(starts, list(starts[1:]) + [runs.size]):
                    state[runs[a:z]] = po.states_before(SYMBOL_ORDER, lens[runs[a:z]])
                    if a > 0:
                        before = po.compose(state[runs[a - 1]][None, :], po.dense(lens[runs[a - 1]][None, :]))[0]
                        cnt["resets_changing"] += int(not np.array_equal(before, SYMBOL_ORDER))
            else:
                state[runs] = carried
            W = state[vs]
            mine = W[np.arange(n), g][:, None]
            k = np.minimum(ln, r[:, None]).sum(axis=1) + ((ln > r[:, None]) & (W < mine)).sum(axis=1)
        elif i == L - BLOCK_PREFIX:
            k = quirk_places(S, g, gstart, vs, lens, lb, base, fk, cnt) if quirk else sym_k
        else:
            k = cat_k if concat else sym_k
        pos = base[vs] + k
        A = np.zeros(n, dtype=np.int64)
        A[pos] = S
        kA = np.zeros(n, dtype=np.int64)
        kA[pos] = k
        vA = np.zeros(n, dtype=np.int64)
        vA[pos] = vs
        lo = np.searchsorted(vp, vA, side="left")
        hi = np.searchsorted(vp, vA, side="right")
        nb = hi - lo
        q = lo + kA
        e = (kA < nb) & (P[np.minimum(q, P.size - 1)] == A)
        run_start = kA == 0
        ev = po.events_closed_form(e, run_start)
        after = np.concatenate([[False], ev[:-1]]) & ~run_start
        cnt["self_conflicts"] += int(ev.sum())
        take = np.where(after, q - 1, np.where(ev, q + 1, q))
        ok = after | np.where(ev, kA + 1 < nb, kA < nb)
        nxt[A[ok]] = P[take[ok]]
        ov[A[ok]] = m
        left -= int(ok.sum())
        taken = np.zeros(P.size, dtype=bool)
        assert np.unique(take[ok]).size == int(ok.sum())
        taken[take[ok]] = True
        gone = ~ok & (kA >= nb) & (hi == P.size)
        cnt["would_drop"] += int(gone.sum())
        S = A[~ok & ~gone] if drop else A[~ok]
        P = P[~taken]
        log.append(left)
    cnt["follower_compares"] = fk.compares
    cnt["past_end_compares"] = fk.past_end
    return {"next_read": nxt, "overlap": ov, "reads_left": np.array(log, dtype=np.uint64), "duplicates": duplicates,
            "links": R - left - duplicates, "sweeps": max(iters - 1, 0), "counters": cnt}


def valid_graph(codes, next_read, overlap):
    """every overlap is real and no read has two predecessors"""
    codes = np.asarray(codes)
    R, L = codes.shape
    nx = np.asarray(next_read, dtype=np.int64)
    ovl = np.asarray(overlap, dtype=np.int64)
    has = np.flatnonzero(nx[1:]) + 1
    if np.unique(nx[has]).size != has.size or (nx[has] > R).any():
        return False
    for x in has:
        m = int(ovl[x])
        if m < 1 or m > L or not np.array_equal(codes[x - 1, L - m:], codes[nx[x] - 1, :m]):
            return False
    return not (ovl[nx == 0] != 0).any()


def random_case(k):
    """pgovl_util.random_case; L is 4 .. 40 there"""
    return po.random_case(k)
