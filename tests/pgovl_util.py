"""Checker of the overlap search (include/pgrc_overlap.h), three things:

  literal          the reference's serial loops as they stand in GreedySwipingPackedOverlapPseudoGenomeGenerator.cpp at one
                   thread: initAndFindDuplicates<false> (:97-136), the sweeps of findOverlappingReads (:139-169) with
                   updateSuffixQueue (:84-95) and overlapSortedReadsAndMergeSortSuffixes<false> (:171-249), and
                   getBothSidesOverlappedReads (AbstractOverlapPseudoGenomeGenerator.cpp:75-91)
  parallel_form    the rule the device runs, in numpy: the merged order of a sweep from ranks inside runs of
                   equal suffixes and a weak order of the five groups folded over the runs with an associative operator (in a
                   tree), the class of a run in the prefix list by search, the pairing by its closed form, the drop rule.
                   Three switches turn it into the three simplifications that are NOT the reference
  the generators   genome-like reads with substitutions, low-complexity periodic reads, tiny alphabets

Reads are numbered 1 .. R (0 = none); next_read and overlap have R + 1 elements.  The order among equal reads is an input
(`order`: the read numbers in sorted order); stable_order gives the one with equal reads in ascending number."""
import numpy as np

from pgasm_util import ALPHABETS, pack_rows, row_bytes, unpack_rows  # noqa: F401  (re-exported for the tests)

GROUPS = 5      # groups of a sweep: one per symbol, 4 or 5 in use


def to_codes(reads, symbols):
    """uint8 [R, L] ASCII -> the symbols' places in the alphabet's order"""
    lut = np.full(256, 255, dtype=np.uint8)
    for k, ch in enumerate(ALPHABETS[symbols]):
        lut[ch] = k
    codes = lut[np.asarray(reads, dtype=np.uint8)]
    assert (codes != 255).all(), "a symbol outside the alphabet"
    return codes


def iterations(L, coef):
    """overlapIterations of :145: the double product cut to uint_read_len (one or two bytes)"""
    return int(float(L) * float(coef)) & (0xFF if L <= 255 else 0xFFFF)


def stable_order(codes):
    """read numbers 1 .. R in sorted order, equal reads in ascending number"""
    R, L = codes.shape
    return (np.lexsort(codes.T[::-1]) + 1).astype(np.uint32) if L else np.arange(1, R + 1, dtype=np.uint32)


def order_is_sorted(codes, order):
    order = np.asarray(order, dtype=np.int64)
    if sorted(order.tolist()) != list(range(1, codes.shape[0] + 1)):
        return False
    rows = [codes[r - 1].tobytes() for r in order]
    return all(a <= b for a, b in zip(rows, rows[1:]))


# ------------------------------------------------------------------------------------------------ the literal loops
def literal(codes, order, coef, symbols=None):
    """-> next_read (uint32 [R + 1]), overlap (uint16 [R + 1]), reads_left (the log's numbers: after the duplicates, then after
    every sweep), duplicates, links, sweeps"""
    codes = np.asarray(codes, dtype=np.uint8)
    R, L = codes.shape
    symbols = symbols or GROUPS
    rows = [codes[r].tobytes() for r in range(R)]

    def suf(r, off):
        return rows[r - 1][off:]

    def cmp_sp(s, p, off):                              # compareSuffixWithPrefix
        a, b = rows[s - 1][off:], rows[p - 1][:L - off]
        return (a > b) - (a < b)

    nxt = np.zeros(R + 1, dtype=np.uint32)
    ov = np.zeros(R + 1, dtype=np.uint16)
    reads_left = R
    # initAndFindDuplicates<false>
    P = [int(x) for x in order]
    S = []
    ssi_idx, ssi_end = [0] * 256, [0] * 256
    cur = 0
    left = 1
    k = 0
    while k < len(P):
        k += 1
        if k < len(P) and rows[P[k - 1] - 1] == rows[P[k] - 1]:
            nxt[P[k - 1]] = P[k]
            ov[P[k - 1]] = L
            reads_left -= 1
        else:
            S.append(P[k - 1])
            first = int(codes[P[k - 1] - 1, 0])
            if cur != first:
                ssi_end[cur] = len(S) - 1
                ssi_idx[first] = len(S) - 1
                cur = first
            if k < len(P):
                P[left] = P[k]
                left += 1
    ssi_end[cur] = len(S)
    del P[left:]
    duplicates = R - reads_left
    log = [reads_left]
    iters = iterations(L, coef)
    for i in range(1, iters):
        # overlapSortedReadsAndMergeSortSuffixes<false>(i)
        kept_p = []
        s_left = []
        idx_left, end_left = [0] * 256, [0] * 256
        cur = 0
        queue = []

        def update(g):
            if ssi_idx[g] < ssi_end[g]:
                mine = suf(S[ssi_idx[g]], i)
                at = len(queue)
                while True:
                    if at == 0 or mine >= suf(S[ssi_idx[queue[at - 1]]], i):
                        queue.insert(at, g)
                        break
                    at -= 1

        for g in range(symbols):
            update(g)
        pre = 0
        while queue or pre < len(P):
            if not queue:
                kept_p.append(P[pre])
                pre += 1
                continue
            g = queue[0]
            s = S[ssi_idx[g]]
            if pre < len(P):
                res = -1
                start = pre
                while pre < len(P):
                    res = cmp_sp(s, P[pre], i)
                    if res != 0:
                        break
                    if s != P[pre]:
                        break
                    res = -1
                    pre += 1
                if res:
                    pre = start
                else:
                    p = P[pre]
                    while pre > start:
                        P[pre] = P[pre - 1]
                        pre -= 1
                    P[pre] = p
                if res == 0:
                    nxt[s] = P[pre]
                    ov[s] = L - i
                    pre += 1
                    reads_left -= 1
                elif res > 0:
                    kept_p.append(P[pre])
                    pre += 1
                    continue
                else:
                    s_left.append(s)
                    sym = int(codes[s - 1, i])
                    if cur != sym:
                        end_left[cur] = len(s_left) - 1
                        idx_left[sym] = len(s_left) - 1
                        cur = sym
            queue.pop(0)
            ssi_idx[g] += 1
            update(g)
        end_left[cur] = len(s_left)
        P = kept_p
        S = s_left
        ssi_idx, ssi_end = idx_left, end_left
        log.append(reads_left)
    return {"next_read": nxt, "overlap": ov, "reads_left": np.array(log, dtype=np.uint64), "duplicates": duplicates,
            "links": R - reads_left - duplicates, "sweeps": max(iters - 1, 0)}


def both_sides(next_read, overlap, L):
    """getBothSidesOverlappedReads: R bytes"""
    nx = np.asarray(next_read, dtype=np.int64)
    ov = np.asarray(overlap, dtype=np.int64)
    R = nx.size - 1
    prev = np.zeros(R + 1, dtype=np.int64)
    has = nx[1:] != 0
    prev[nx[1:][has]] = ov[1:][has]
    res = np.ones(R, dtype=np.uint8)
    for i in range(1, R + 1):
        if prev[i] and nx[i]:
            continue
        if nx[i] and ov[i] == L:
            continue
        if prev[i] == L:
            continue
        res[i - 1] = 0
    return res


# ------------------------------------------------------------------------------------------------ the parallel form
SYMBOL_ORDER = np.arange(GROUPS, dtype=np.int64)


def dense(keys):
    """[n, 5] keys -> dense ranks per row: the number of distinct smaller keys"""
    keys = np.asarray(keys, dtype=np.int64)
    out = np.zeros_like(keys)
    for h in range(GROUPS):
        first = np.ones(keys.shape[0], dtype=bool)
        for h2 in range(h):
            first &= keys[:, h2] != keys[:, h]
        for g in range(GROUPS):
            out[:, g] += first & (keys[:, h] < keys[:, g])
    return out


def compose(w1, w2):
    """the weak order after w1 and then w2: dense ranks of the pairs (w2[g], w1[g]); associative, the all-equal order is
    its identity"""
    return dense(np.asarray(w2, dtype=np.int64) * 8 + np.asarray(w1, dtype=np.int64))


def compose_steps(seed, keys):
    """the step-by-step form: the state in front of every transition"""
    out = np.zeros((len(keys), GROUPS), dtype=np.int64)
    w = np.asarray(seed, dtype=np.int64)[None, :]
    for k in range(len(keys)):
        out[k] = w[0]
        w = compose(w, dense(keys[k:k + 1]))
    return out


def states_before(seed, keys):
    """[n, 5] key vectors of n transitions -> the state in front of each: an exclusive scan with compose, seeded; the fold is
    a tree (doubling distances)"""
    n = keys.shape[0]
    inc = dense(keys)
    d = 1
    while d < n:
        inc = np.concatenate([inc[:d], compose(inc[:-d], inc[d:])])
        d *= 2
    seed = np.asarray(seed, dtype=np.int64)[None, :]
    out = np.repeat(seed, n, axis=0)
    if n > 1:
        out[1:] = compose(np.repeat(seed, n - 1, axis=0), inc[:-1])
    return out


def events_closed_form(e, run_start):
    """e[k] over positions in merged order, run_start[k] = True at a run's first position -> event[k] = e[k] and not
    event[k - 1] inside a run: inside a streak of e the events alternate from its first position"""
    n = e.size
    idx = np.arange(n)
    prev_e = np.concatenate([[False], e[:-1]]) & ~run_start
    begins = e & ~prev_e
    last = np.maximum.accumulate(np.where(begins, idx, 0))
    return e & ((idx - last) % 2 == 0)


def events_automaton(e, run_start):
    ev = np.zeros(e.size, dtype=bool)
    for k in range(e.size):
        ev[k] = e[k] and not (k > 0 and not run_start[k] and ev[k - 1])
    return ev


def joint_ranks(codes, S, P, i):
    """dense ranks of suf_i of the reads of S and of pre_(L - i) of the reads of P, comparable with one another"""
    L = codes.shape[1]
    m = L - i
    a = np.ascontiguousarray(codes[S - 1, i:] + 1)
    b = np.ascontiguousarray(codes[P - 1, :m] + 1)
    both = np.ascontiguousarray(np.concatenate([a, b])).view("S%d" % m).ravel()
    _, inv = np.unique(both, return_inverse=True)
    inv = inv.ravel()
    return inv[:S.size], inv[S.size:]


def parallel_form(codes, order, coef, ties="state", round_robin=True, drop=True):
    """as literal; also `counters`: tie_runs (runs shared by groups), tie_runs_off_symbol_order, round_robin_runs,
    self_conflicts, dropped.  ties="symbol", round_robin=False and drop=False are the three simplifications"""
    codes = np.asarray(codes, dtype=np.uint8)
    R, L = codes.shape
    order = np.asarray(order, dtype=np.int64)
    nxt = np.zeros(R + 1, dtype=np.uint32)
    ov = np.zeros(R + 1, dtype=np.uint16)
    # start: runs of equal reads become chains
    rows = np.ascontiguousarray(codes[order - 1] + 1).view("S%d" % L).ravel()
    same = rows[:-1] == rows[1:]                            # order[j] equals order[j + 1]
    nxt[order[:-1][same]] = order[1:][same]
    ov[order[:-1][same]] = L
    P = order[np.concatenate([[True], ~same])]
    S = order[np.concatenate([~same, [True]])]
    duplicates = int(same.sum())
    left = R - duplicates
    log = [left]
    cnt = dict(tie_runs=0, tie_runs_off_symbol_order=0, round_robin_runs=0, self_conflicts=0, dropped=0)
    iters = iterations(L, coef)
    for i in range(1, iters):
        if S.size == 0 or P.size == 0:
            cnt["dropped"] += int(S.size) if drop else 0
            if drop:
                S = S[:0]
            log.append(left)
            continue
        m = L - i
        vs, vp = joint_ranks(codes, S, P, i)
        n = S.size
        g = codes[S - 1, i - 1].astype(np.int64)            # the group: S is sorted by suf_(i-1), the groups are contiguous
        gstart = np.searchsorted(g, np.arange(GROUPS), side="left")
        nv = int(max(vs.max(), vp.max())) + 1
        lens = np.zeros((nv, GROUPS), dtype=np.int64)
        np.add.at(lens, (vs, g), 1)
        lb = np.cumsum(lens, axis=0) - lens                 # per group: suffixes below the value
        base = np.cumsum(lens.sum(axis=1)) - lens.sum(axis=1)
        r = (np.arange(n) - gstart[g]) - lb[vs, g]          # rank inside the group's part of the run
        runs = np.flatnonzero(lens.sum(axis=1) > 0)
        state = np.repeat(SYMBOL_ORDER[None, :], nv, axis=0)
        if ties == "state":
            state[runs] = states_before(SYMBOL_ORDER, lens[runs])
        W = state[vs]                                       # the state in front of the element's run
        ln = lens[vs]
        part = ln > 0
        mine = W[np.arange(n), g][:, None]
        if round_robin:
            k = np.minimum(ln, r[:, None]).sum(axis=1) + ((ln > r[:, None]) & (W < mine)).sum(axis=1)
        else:
            k = (ln * (part & (W < mine))).sum(axis=1) + r
        pos = base[vs] + k
        A = np.zeros(n, dtype=np.int64)
        A[pos] = S
        kA = np.zeros(n, dtype=np.int64)
        kA[pos] = k
        vA = np.zeros(n, dtype=np.int64)
        vA[pos] = vs
        # counters of the merged order
        shared = (lens[runs] > 0).sum(axis=1) >= 2
        cnt["tie_runs"] += int(shared.sum())
        st = state[runs]
        for t in np.flatnonzero(shared):
            gs = np.flatnonzero(lens[runs[t]] > 0)
            cnt["tie_runs_off_symbol_order"] += int((np.diff(st[t][gs]) < 0).any())
        cnt["round_robin_runs"] += int((shared & (lens[runs].max(axis=1) >= 2)).sum())
        # classes and the pairing
        lo = np.searchsorted(vp, vA, side="left")
        hi = np.searchsorted(vp, vA, side="right")
        nb = hi - lo
        q = lo + kA
        e = (kA < nb) & (P[np.minimum(q, P.size - 1)] == A)
        run_start = kA == 0
        ev = events_closed_form(e, run_start)
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
        gone = ~ok & (kA >= nb) & (hi == P.size) if drop else np.zeros(n, dtype=bool)
        cnt["dropped"] += int(gone.sum())
        S = A[~ok & ~gone]
        P = P[~taken]
        log.append(left)
    return {"next_read": nxt, "overlap": ov, "reads_left": np.array(log, dtype=np.uint64), "duplicates": duplicates,
            "links": R - left - duplicates, "sweeps": max(iters - 1, 0), "counters": cnt}


def same_result(a, b):
    return (np.array_equal(a["next_read"], b["next_read"]) and np.array_equal(a["overlap"], b["overlap"])
            and np.array_equal(a["reads_left"], b["reads_left"]) and (a["duplicates"], a["links"], a["sweeps"]) == (b["duplicates"], b["links"], b["sweeps"]))


# ------------------------------------------------------------------------------------------------ the generators
def ascii_of(codes, symbols):
    return np.frombuffer(ALPHABETS[symbols], dtype=np.uint8)[codes]


def gen_genome(rng, R, L, symbols, coverage=30.0, subst=0.01, dup=0.02, letters=None):
    """reads from a random text at the given coverage with substitutions, a share of them repeated -> codes [R, L]"""
    letters = letters or symbols
    glen = max(L + 1, int(R * L / coverage))
    genome = rng.integers(0, letters, size=glen).astype(np.uint8)
    if symbols == 5 and letters == 5:
        genome = np.where(genome == 3, rng.integers(0, 5, size=glen), genome).astype(np.uint8)   # (N is rarer)
    pos = rng.integers(0, glen - L + 1, size=R)
    reads = genome[pos[:, None] + np.arange(L)[None, :]].copy()
    err = rng.random(reads.shape) < subst
    reads[err] = rng.integers(0, letters, size=int(err.sum())).astype(np.uint8)
    ndup = int(R * dup)
    if ndup and R > 1:
        reads[rng.integers(0, R, size=ndup)] = reads[rng.integers(0, R, size=ndup)]
    return reads


def gen_periodic(rng, R, L, symbols, max_period=4, letters=2):
    """low-complexity reads: a short unit repeated from a random phase, a few with one substitution"""
    reads = np.zeros((R, L), dtype=np.uint8)
    for k in range(R):
        p = int(rng.integers(1, max_period + 1))
        unit = rng.integers(0, letters, size=p).astype(np.uint8)
        reads[k] = unit[(np.arange(L) + int(rng.integers(0, p))) % p]
        if rng.random() < 0.2:
            reads[k, int(rng.integers(0, L))] = rng.integers(0, min(symbols, letters + 1))
    return reads


def gen_mixed(rng, R, L, symbols):
    """genome-like, periodic and two-letter reads in one set"""
    a = R // 2
    b = (R - a) // 2
    parts = [gen_genome(rng, a, L, symbols, coverage=float(rng.choice([8, 30]))) if a else np.zeros((0, L), np.uint8),
             gen_periodic(rng, b, L, symbols, letters=int(rng.integers(1, 4))) if b else np.zeros((0, L), np.uint8),
             gen_genome(rng, R - a - b, L, symbols, coverage=20.0, subst=0.02, letters=2) if R - a - b else np.zeros((0, L), np.uint8)]
    reads = np.concatenate(parts)
    return reads[rng.permutation(R)]


def random_case(k):
    """a fixed-seed setting of the CPU sweep: -> codes, symbols, coef, order (sorted, equal reads in a random order)"""
    rng = np.random.default_rng(5000 + k)
    symbols = 4 if k % 2 else 5
    L = int(rng.integers(4, 41))
    R = int(rng.integers(1, 400))
    kind = k % 3
    if kind == 0:
        codes = gen_genome(rng, R, L, symbols, coverage=float(rng.choice([5, 30, 100])), subst=float(rng.choice([0, 0.01, 0.05])))
    elif kind == 1:
        codes = gen_periodic(rng, R, L, symbols, max_period=int(rng.integers(1, 6)), letters=int(rng.integers(1, 4)))
    else:
        codes = gen_mixed(rng, R, L, symbols)
    coef = float(rng.choice([1.0, 0.75, 0.5]))
    return codes, symbols, coef, shuffled_order(rng, codes)


def shuffled_order(rng, codes):
    """a sorted order whose equal reads stand in a random order, as an unstable sort may leave them"""
    R = codes.shape[0]
    perm = rng.permutation(R)
    return (perm[np.lexsort(codes[perm].T[::-1])] + 1).astype(np.uint32)
