"""Checkers of the reads list on the device (include/pgrc_readslist.h): the position array of the order-preserving paired
mode (orgIdx2PgPos) restated twice -- the reference's loops copied line by line, and with numpy -- and seeded settings for it."""
import numpy as np

NOT_MATCHED = 2**64 - 1
FILL = np.uint64(NOT_MATCHED)          # vector<uint_pg_len_max>(readsTotalCount, -1)


def positions_literal(T, hq, lq, nn, hq_len, lq_len, read_org=None, match_pos=None):
    """hq, lq, nn: (off, orgIdx) of a reads list or None; read_org / match_pos: the matcher's reads.  The loops of
    ReadsMatchers.cpp:604-610 and :659 and of pgrc-encoder.cpp:173-178 and :193-198, in the reference's order."""
    arr = [NOT_MATCHED] * T
    off, org = hq
    pos = 0
    for i in range(len(org)):
        pos += int(off[i])
        arr[int(org[i])] = pos
    if match_pos is not None:
        for i in range(len(match_pos)):
            o_idx = int(read_org[i]) if read_org is not None else i
            if int(match_pos[i]) != NOT_MATCHED:
                arr[o_idx] = int(match_pos[i])
    if lq is not None:
        off, org = lq
        pos = hq_len
        for i in range(len(org)):
            pos += int(off[i])
            arr[int(org[i])] = pos
    if nn is not None:
        off, org = nn
        pos = hq_len + lq_len
        for i in range(len(org)):
            pos += int(off[i])
            arr[int(org[i])] = pos
    return np.array(arr, dtype=np.uint64)


def positions_numpy(T, hq, lq, nn, hq_len, lq_len, read_org=None, match_pos=None):
    """The same as scans and scatters.  Valid where every index is written at most once (then the order of the writes does not
    matter); writers_per_index tells."""
    arr = np.full(T, FILL, dtype=np.uint64)
    for lst, base in ((hq, 0), (lq, hq_len), (nn, hq_len + lq_len)):
        if lst is None:
            continue
        off, org = lst
        arr[np.asarray(org, dtype=np.int64)] = np.uint64(base) + np.cumsum(np.asarray(off, dtype=np.uint64), dtype=np.uint64)
    if match_pos is not None:
        mp = np.asarray(match_pos, dtype=np.uint64)
        hit = mp != FILL
        ro = np.arange(mp.size) if read_org is None else np.asarray(read_org, dtype=np.int64)
        arr[ro[hit]] = mp[hit]
    return arr


def writers_per_index(T, hq, lq, nn, read_org=None, match_pos=None):
    """how often every index in [0, T) is written (an index of T or more raises)"""
    idx = [np.asarray(l[1], dtype=np.int64) for l in (hq, lq, nn) if l is not None]
    if match_pos is not None:
        mp = np.asarray(match_pos, dtype=np.uint64)
        ro = np.arange(mp.size) if read_org is None else np.asarray(read_org, dtype=np.int64)
        idx.append(ro[mp != FILL])
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    if idx.size and int(idx.max()) >= T:
        raise IndexError("an index of T or more")
    return np.bincount(idx, minlength=T)


def make_setting(seed, T=None, hq_len=None, max_off=300):
    """a seeded setting: a permutation of [0, T) dealt to the HQ list, the matcher's matched reads, the LQ and the N list
    (any of the last three may be empty or absent), offsets below max_off, hq_len / lq_len at least the lists' spans"""
    rng = np.random.default_rng(seed)
    if T is None:
        T = 2 * int(rng.choice([1, 2, int(rng.integers(3, 40)), int(rng.integers(40, 3000))]))
    perm = rng.permutation(T).astype(np.uint32)
    cuts = np.sort(rng.integers(0, T + 1, size=3))
    kind = int(rng.integers(0, 4))
    if kind == 0:
        cuts[:] = T                         # everything in the HQ list
    elif kind == 1:
        cuts[1] = cuts[2] = T               # no LQ and no N entries: the matcher's reads carry the rest
    parts = [perm[: cuts[0]], perm[cuts[0]: cuts[1]], perm[cuts[1]: cuts[2]], perm[cuts[2]:]]       # hq, matched, lq, n

    def lst(org):
        return rng.integers(0, max_off, size=org.size).astype(np.uint16), org.copy()
    hq, lq, nn = lst(parts[0]), lst(parts[2]), lst(parts[3])
    span = [int(l[0].sum(dtype=np.int64)) for l in (hq, lq, nn)]
    if hq_len is None:
        hq_len = span[0] + 100 if seed % 3 else (1 << 32) - int(rng.integers(0, max(2, span[1] + 2)))       # LQ positions on both sides of 2^32
    hq_len = max(hq_len, span[0] + 100)
    lq_len = span[1] + int(rng.integers(0, 200))
    # the matcher: its matched reads carry parts[1], a few unmatched reads carry indexes that stay out of the way (>= T is
    # never looked at: an unmatched read writes nothing)
    n_un = int(rng.integers(0, 5))
    read_org = np.concatenate([parts[1], rng.integers(0, max(T, 1), size=n_un).astype(np.uint32)])
    match_pos = np.concatenate([rng.integers(0, max(hq_len, 1), size=parts[1].size).astype(np.uint64), np.full(n_un, FILL, dtype=np.uint64)])
    order = rng.permutation(read_org.size)
    return {"T": T, "hq": hq, "lq": lq if kind != 1 or seed % 2 else None, "n": nn if kind != 1 or seed % 2 else None, "hq_len": int(hq_len), "lq_len": int(lq_len),
            "read_org": read_org[order], "match_pos": match_pos[order]}


def positions_of(s, fn):
    return fn(s["T"], s["hq"], s["lq"], s["n"], s["hq_len"], s["lq_len"], s["read_org"], s["match_pos"])
