"""Checker of the pseudogenome assembly (include/pgrc_assemble.h), three things:

  literal_*        the reference's loops as they stand in AbstractOverlapPseudoGenomeGenerator.cpp: the cycle removal with getHead's
                   path compression and the two shadowed locals of :20-21 (:6-41), the length count (:146-153), the assembly with
                   prefixDoneLength (:183-219, GeneratedSeparatedPseudoGenome::append) and applyIndexesMapping
  parallel_form    the closed form the device runs, in numpy: cuts at the largest index of a cycle, heads and distances by
                   pointer jumping, places by a scan of the chain lengths, every entry's first `shift` symbols at the scan
                   of the shifts
  make_case        consistent cases from any graph: a random text per chain (circular for a cycle), reads cut at the shifts,
                   read ids by a random permutation

Reads are numbered 1 .. R (0 = no successor); next_read and overlap have R + 1 elements."""
import numpy as np

ALPHABETS = {4: b"ACGT", 5: b"ACGNT"}


# ------------------------------------------------------------------------------------------------ packing
def row_bytes(L, symbols):
    return (L + 3) // 4 if symbols == 4 else (L + 2) // 3


def pack_rows(reads, symbols):
    """SymbolsPackingFacility::packSequence of every row of the uint8 [R, L] ASCII array: big-endian digits, a last partial
    byte padded with zero digits"""
    reads = np.asarray(reads, dtype=np.uint8)
    R, L = reads.shape
    lut = np.full(256, 255, dtype=np.uint8)
    for k, ch in enumerate(ALPHABETS[symbols]):
        lut[ch] = k
    codes = lut[reads]
    assert (codes != 255).all(), "a symbol outside the alphabet"
    spb = 4 if symbols == 4 else 3
    rb = row_bytes(L, symbols)
    pad = np.zeros((R, rb * spb), dtype=np.uint16)
    pad[:, :L] = codes
    pad = pad.reshape(R, rb, spb)
    w = np.array([64, 16, 4, 1] if symbols == 4 else [25, 5, 1], dtype=np.uint16)
    return (pad * w).sum(axis=2).astype(np.uint8)


def unpack_rows(rows, L, symbols):
    rows = np.asarray(rows, dtype=np.uint8)
    R = rows.shape[0]
    v = rows.astype(np.uint16)
    if symbols == 4:
        d = np.stack([(v >> 6) & 3, (v >> 4) & 3, (v >> 2) & 3, v & 3], axis=2)
    else:
        d = np.stack([v // 25, (v // 5) % 5, v % 5], axis=2)
    return np.frombuffer(ALPHABETS[symbols], dtype=np.uint8)[d.reshape(R, -1)[:, :L]]


# ------------------------------------------------------------------------------------------------ the literal loops
def literal_remove_cycles(next_read, overlap):
    """removeCyclesAndPrepareComponents -> (nextRead, overlap, headRead, cycles, overlapLost, cuts); headRead non-zero = "has a
    predecessor"; cuts: the reads whose link was cut, in the loop's order"""
    nx = [int(x) for x in next_read]
    ov = [int(x) for x in overlap]
    R = len(nx) - 1
    head = [0] * (R + 1)

    def get_head(idx):
        path = []
        while head[idx]:
            path.append(idx)
            idx = head[idx]
        for p in path:
            head[p] = idx
        return idx

    cycles = lost = 0
    cuts = []
    for cur in range(1, R + 1):
        nxt = nx[cur]
        if not nxt:
            continue
        if get_head(cur) == nxt:
            cycles += 1
            min_overlap, min_idx = ov[cur], cur
            k = cur
            while True:
                k = nx[k]
                if k == cur:
                    break
                if min_overlap > ov[k]:
                    shadow_overlap, shadow_idx = ov[k], k       # the two locals of :20-21 shadow the outer ones  # noqa: F841
            lost += min_overlap
            head_idx = nx[min_idx]
            nx[min_idx] = 0
            ov[min_idx] = 0
            cuts.append(min_idx)
            k = head_idx
            head[head_idx] = 0
            while True:
                k = nx[k]
                if not k:
                    break
                head[k] = head_idx
        else:
            head[nxt] = cur if head[cur] == 0 else head[cur]
    dt = np.asarray(overlap).dtype
    return np.array(nx, dtype=np.uint32), np.array(ov, dtype=dt), np.array(head, dtype=np.uint32), cycles, lost, cuts


def literal_assemble(reads, next_read, overlap, head, mapping=None):
    """countPseudoGenomeLength, quick_stats' two counts, assemblePseudoGenomeTemplate<GeneratedSeparatedPseudoGenome> and
    applyIndexesMapping, after the cuts.  reads: uint8 [R, L] ASCII."""
    reads = np.asarray(reads, dtype=np.uint8)
    R, L = reads.shape
    nx = [int(x) for x in next_read]
    ov = [int(x) for x in overlap]
    hd = [int(x) for x in head]
    pg_len = sum(L - ov[i] for i in range(1, R + 1) if ov[i] < L)
    components = sum(1 for i in range(1, R + 1) if not hd[i] and nx[i])
    singles = sum(1 for i in range(1, R + 1) if not hd[i] and not nx[i])
    seq = np.zeros(pg_len, dtype=np.uint8)
    off, org = [], []
    pos = delta = done = 0
    for i in range(1, R + 1):
        if hd[i]:
            continue
        idx = i
        while idx:
            off.append(delta)
            org.append(idx - 1)
            delta = L - ov[idx]
            if done < delta:
                seq[pos:pos + L - done] = reads[idx - 1, done:]
                pos += L - done
                done = ov[idx]
            else:
                done -= delta
            idx = nx[idx]
    assert pos == pg_len and len(org) == R
    org = np.array(org, dtype=np.uint32)
    if mapping is not None:
        org = np.asarray(mapping, dtype=np.uint32)[org]
    return {"text": seq, "off": np.array(off, dtype=np.uint16), "org_idx": org, "pg_len": pg_len, "components": components, "singles": singles}


def literal(reads, next_read, overlap, mapping=None):
    """everything after findOverlappingReads, as the reference computes it"""
    nx, ov, head, cycles, lost, cuts = literal_remove_cycles(next_read, overlap)
    out = literal_assemble(reads, nx, ov, head, mapping)
    out.update(cycles=cycles, overlap_lost=lost, cuts=cuts, next_read=nx, overlap=ov)
    return out


# ------------------------------------------------------------------------------------------------ the parallel form
def parallel_form(reads, next_read, overlap, mapping=None):
    reads = np.asarray(reads, dtype=np.uint8)
    R, L = reads.shape
    nx = np.asarray(next_read, dtype=np.int64).copy()
    ov = np.asarray(overlap, dtype=np.int64).copy()
    nx[0] = ov[0] = 0
    idx = np.arange(R + 1, dtype=np.int64)
    # cycles: jumping on next with the running maximum; what is live after the passes lies on a cycle
    ptr, mx = nx.copy(), idx.copy()
    for _ in range(int(np.ceil(np.log2(R + 1))) + 1):
        live = ptr != 0
        if not live.any():
            break
        mx = np.where(live, np.maximum(mx, mx[ptr]), mx)
        ptr = np.where(live, ptr[ptr], ptr)
    cut = np.flatnonzero((ptr != 0) & (mx == idx))
    cycles, lost = cut.size, int(ov[cut].sum())
    nx[cut] = 0
    ov[cut] = 0
    # ranking: pred, then (head, distance) by jumping
    pred = np.zeros(R + 1, dtype=np.int64)
    src = np.flatnonzero(nx)
    pred[nx[src]] = src
    head = np.where(pred != 0, pred, idx)
    dist = (pred != 0).astype(np.int64)
    while True:
        hh = head[head]
        move = hh != head
        if not move.any():
            break
        dist = np.where(move, dist + dist[head], dist)
        head = hh
    tails = np.flatnonzero(nx[1:] == 0) + 1
    length = np.zeros(R + 1, dtype=np.int64)
    length[head[tails]] = dist[tails] + 1
    base = np.cumsum(length) - length
    place = base[head[1:]] + dist[1:]
    walk = np.empty(R, dtype=np.int64)
    walk[place] = idx[1:]
    shift = L - ov[walk]
    off = np.concatenate(([0], shift[:-1])).astype(np.uint16)
    org = (walk - 1).astype(np.uint32)
    if mapping is not None:
        org = np.asarray(mapping, dtype=np.uint32)[org]
    start = np.cumsum(shift) - shift
    pg_len = int(shift.sum())
    # every entry's first `shift` symbols at its start
    ent = np.repeat(np.arange(R), shift)
    col = np.arange(pg_len) - np.repeat(start, shift)
    text = reads[walk[ent] - 1, col]
    is_head = (head[1:] == idx[1:])
    return {"text": text, "off": off, "org_idx": org, "pg_len": pg_len, "cycles": cycles, "overlap_lost": lost,
            "components": int((is_head & (nx[1:] != 0)).sum()), "singles": int((is_head & (nx[1:] == 0)).sum()),
            "cuts": sorted(int(c) for c in cut)}


# ------------------------------------------------------------------------------------------------ cases
def make_case(seed, L, symbols=4, chains=(), cycles=(), singles=0, dup=0.0, mean_shift=None, n_share=0.0, shuffle=True, ov_dtype=np.uint8):
    """A consistent case: `chains` and `cycles` are lists of lengths in reads, `singles` a count.  Every chain gets a random text
    and its reads start at the running sum of random shifts in [1, L] (mean about mean_shift; 0 with probability `dup`: a
    duplicate of the read before); a cycle's text is circular -- the shifts add up to its length, which may be shorter than L
    -- and its last read links back to its first.  With 5 symbols a share n_share of the text is N.  Read ids come from a
    random permutation.  -> dict(reads [R, L] ASCII, rows, next_read, overlap, L, symbols)"""
    rng = np.random.default_rng(seed)
    mean_shift = mean_shift or max(1, L // 4)
    sizes = [int(c) for c in chains] + [int(c) for c in cycles] + [1] * int(singles)
    kinds = [0] * len(chains) + [1] * len(cycles) + [0] * int(singles)
    R = sum(sizes)
    alpha = np.frombuffer(ALPHABETS[symbols], dtype=np.uint8)
    letters = alpha if symbols == 4 else alpha[[0, 1, 2, 4]]
    ids = (rng.permutation(R) if shuffle else np.arange(R)) + 1
    reads = np.empty((R, L), dtype=np.uint8)
    nx = np.zeros(R + 1, dtype=np.uint32)
    ov = np.zeros(R + 1, dtype=ov_dtype)
    first = 0
    for size, cyc in zip(sizes, kinds):
        my = ids[first:first + size]
        first += size
        shifts = np.minimum(rng.geometric(1.0 / mean_shift, size=size), L)
        shifts[rng.random(size) < dup] = 0
        if cyc:
            if shifts.sum() == 0:
                shifts[-1] = 1
            tlen = int(shifts.sum())
        else:
            shifts[-1] = L                                      # (the tail: overlap 0)
            tlen = int(shifts[:-1].sum()) + L
        text = letters[rng.integers(0, 4, size=tlen)]
        if symbols == 5 and n_share:
            text = np.where(rng.random(tlen) < n_share, np.uint8(ord("N")), text)
        starts = np.cumsum(shifts) - shifts
        cols = starts[:, None] + np.arange(L)[None, :]
        reads[my - 1] = text[cols % tlen] if cyc else text[cols]
        nx[my[:-1]] = my[1:]
        ov[my] = L - shifts
        if cyc:
            nx[my[-1]] = my[0]
    return {"reads": reads, "rows": pack_rows(reads, symbols), "next_read": nx, "overlap": ov, "L": L, "symbols": symbols}


def links_are_real(reads, next_read, overlap):
    reads = np.asarray(reads)
    L = reads.shape[1]
    for i in np.flatnonzero(np.asarray(next_read)[1:]) + 1:
        o, n = int(overlap[i]), int(next_read[i])
        if o and not np.array_equal(reads[i - 1, L - o:], reads[n - 1, :o]):
            return False
    return True
