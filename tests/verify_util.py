"""CPU restatement of the verifier (include/pgrc_verify.h, pgrc_amd/csrc/verify.hip) in numpy: the item key bit for bit, the
pairing of the sorted union under given keys, and the two rules themselves -- verify_in_order and verify_multiset, which know
no keys (multiplicities from np.unique) and return the result dict pgrc_amd.Verifier.finish() returns.  Helpers cut rows
and FASTQ text into pieces and feed them to a verifier."""
import numpy as np

IN_ORDER, MULTISET = 1, 2
NONE64, NONE32 = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF
VF_K = np.uint64(0x9E3779B97F4A7C15)
VF_SALT_STEP = 0xD6E8FEB86659FD93
_M1, _M2 = np.uint64(0xFF51AFD7ED558CCD), np.uint64(0xC4CEB9FE1A85EC53)
_S33 = np.uint64(33)


def fmix64(k):
    """MurmurHash3's 64-bit finalizer over a uint64 array"""
    k = np.asarray(k, dtype=np.uint64).copy()
    k ^= k >> _S33
    k *= _M1
    k ^= k >> _S33
    k *= _M2
    k ^= k >> _S33
    return k


def items_of(files):
    """the items of one side: row r of every file side by side, (min rows, F * L) uint8; rows come with or without '\\n'"""
    n = min(f.shape[0] for f in files)
    return np.ascontiguousarray(np.concatenate([np.asarray(f, np.uint8)[:n] for f in files], axis=1))


def hash_items(items, salt=0, bits=64):
    """key = fmix64(salt * STEP + sum_j fmix64(w_j + (j + 1) * K)) over the item's little-endian 8-byte words, the last one
    zero-padded; all sums modulo 2^64; the low `bits` bits"""
    items = np.asarray(items, np.uint8)
    n, B = items.shape
    nw = (B + 7) // 8
    pad = np.zeros((n, nw * 8), np.uint8)
    pad[:, :B] = items
    w = pad.view("<u8")
    acc = np.zeros(n, np.uint64)
    for j in range(nw):
        acc += fmix64(w[:, j] + np.uint64(((j + 1) * int(VF_K)) & NONE64))
    key = fmix64(acc + np.uint64((salt * VF_SALT_STEP) & NONE64))
    return key if bits >= 64 else key & np.uint64((1 << bits) - 1)


def hash_item_loop(item, salt=0):
    """the same for one item with Python integers"""
    def fm(k):
        k ^= k >> 33
        k = (k * 0xFF51AFD7ED558CCD) & NONE64
        k ^= k >> 33
        k = (k * 0xC4CEB9FE1A85EC53) & NONE64
        return k ^ (k >> 33)
    b = bytes(item)
    acc = 0
    for j in range((len(b) + 7) // 8):
        w = int.from_bytes(b[8 * j: 8 * j + 8], "little")
        acc = (acc + fm((w + (j + 1) * 0x9E3779B97F4A7C15) & NONE64)) & NONE64
    return fm((acc + salt * VF_SALT_STEP) & NONE64)


def pair_under_keys(keys_s, items_s, keys_d, items_d):
    """phases 2-4 as the device runs them: a stable sort of the union (source first), offset o of one side of a run of
    equal keys pairs with offset o of the other, pairs are compared byte for byte
    -> (matched, undecided, source_unmatched, decoded_unmatched, first_source_unmatched, first_decoded_unmatched)"""
    ns, nd = len(keys_s), len(keys_d)
    res = [0, 0, 0, 0, NONE64, NONE64]
    runs = {}
    for i, k in enumerate(np.asarray(keys_s, np.uint64).tolist()):
        runs.setdefault(k, ([], []))[0].append(i)
    for i, k in enumerate(np.asarray(keys_d, np.uint64).tolist()):
        runs.setdefault(k, ([], []))[1].append(i)
    for s, d in runs.values():
        for a, b in zip(s, d):
            res[0 if np.array_equal(items_s[a], items_d[b]) else 1] += 1
        for a in s[len(d):]:
            res[2] += 1
            res[4] = min(res[4], a)
        for b in d[len(s):]:
            res[3] += 1
            res[5] = min(res[5], b)
    assert res[0] + res[1] + res[2] == ns and res[0] + res[1] + res[3] == nd
    return tuple(res)


def _result(kind, src_files, dec_files):
    ns = [int(f.shape[0]) for f in src_files] + [0] * (2 - len(src_files))
    nd = [int(f.shape[0]) for f in dec_files] + [0] * (2 - len(dec_files))
    return {"kind": kind, "ok": ns == nd, "salts_used": 0, "n_source": ns, "n_decoded": nd, "mismatched_rows": 0,
            "first_mismatch_file": NONE32, "first_mismatch_row": NONE64, "source_unmatched": 0, "decoded_unmatched": 0,
            "undecided": 0, "first_source_unmatched": NONE64, "first_decoded_unmatched": NONE64}


def _no_newline(files, L):
    return [np.asarray(f, np.uint8).reshape(-1, f.shape[1] if f.ndim == 2 else L)[:, :L] for f in files]


def verify_in_order(src_files, dec_files, L=None):
    """row r of every source file against row r of the job's file, over the rows both have.  Files are (n, L) arrays (the
    job's rows may carry their '\\n': L columns are looked at)"""
    L = src_files[0].shape[1] if L is None else L
    src, dec = _no_newline(src_files, L), _no_newline(dec_files, L)
    r = _result(IN_ORDER, src, dec)
    first = None
    for f, (s, d) in enumerate(zip(src, dec)):
        m = min(s.shape[0], d.shape[0])
        bad = np.flatnonzero((s[:m] != d[:m]).any(axis=1))
        r["mismatched_rows"] += int(bad.size)
        if bad.size and (first is None or (int(bad[0]), f) < first):
            first = (int(bad[0]), f)
    if first is not None:
        r["first_mismatch_row"], r["first_mismatch_file"] = first
    r["ok"] = r["ok"] and r["mismatched_rows"] == 0
    return r


def verify_multiset(src_files, dec_files, L=None):
    """the source items and the job's items as multisets: of m equal source items and k < m equal decoded ones the LAST
    m - k source items (by index) are unmatched, and the other way round.  salts_used is what a run without a collision of
    keys reports: 1, or 0 when neither side has an item"""
    L = src_files[0].shape[1] if L is None else L
    src, dec = _no_newline(src_files, L), _no_newline(dec_files, L)
    r = _result(MULTISET, src, dec)
    S, D = items_of(src), items_of(dec)
    ns, nd = S.shape[0], D.shape[0]
    r["salts_used"] = 1 if ns + nd else 0
    if ns + nd:
        _, inv = np.unique(np.concatenate([S, D]), axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        cs, cd = np.bincount(inv[:ns], minlength=inv.max() + 1), np.bincount(inv[ns:], minlength=inv.max() + 1)

        def unmatched(ids, other):      # occurrence number of every item among its equals, in index order
            order = np.argsort(ids, kind="stable")
            start = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=other.size))])[ids[order]]
            occ = np.empty(ids.size, np.int64)
            occ[order] = np.arange(ids.size) - start
            return np.flatnonzero(occ >= other[ids])
        us, ud = unmatched(inv[:ns], cd), unmatched(inv[ns:], cs)
        r["source_unmatched"], r["decoded_unmatched"] = int(us.size), int(ud.size)
        if us.size:
            r["first_source_unmatched"] = int(us[0])
        if ud.size:
            r["first_decoded_unmatched"] = int(ud[0])
    r["ok"] = r["ok"] and r["source_unmatched"] == 0 and r["decoded_unmatched"] == 0
    return r


def reference(kind, src_files, dec_files, L=None):
    return (verify_in_order if kind == IN_ORDER else verify_multiset)(src_files, dec_files, L)


# ---------------------------------------------------------------- the 20-bit collision case
COLLISION_N, COLLISION_L, COLLISION_BITS = 1000, 16, 20


def collision_case(seed):
    """1000 distinct rows of 16 symbols (the job's rows, in this order) and a permutation: source row i is row perm[i]"""
    rng = np.random.default_rng(seed)
    while True:
        rows = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(COLLISION_N, COLLISION_L))]
        if np.unique(rows, axis=0).shape[0] == COLLISION_N:
            break
    return rows, rng.permutation(COLLISION_N)


def collision_salts(seed):
    """undecided pairs of the case under salt 0, 1 and 2 with the keys cut to 20 bits"""
    rows, perm = collision_case(seed)
    src = rows[perm]
    return [pair_under_keys(hash_items(src, s, COLLISION_BITS), src, hash_items(rows, s, COLLISION_BITS), rows)[1] for s in range(3)]


def find_collision_seed(limit=400):
    """the first seed whose case leaves undecided pairs under salt 0 and none under salt 1"""
    for seed in range(limit):
        u = collision_salts(seed)
        if u[0] > 0 and u[1] == 0:
            return seed
    return None


# ---------------------------------------------------------------- pieces
def cut_points(n, sizes):
    """[0, ..., n]: pieces of the given sizes in turn (repeated) until n is reached"""
    cuts, k = [0], 0
    while cuts[-1] < n:
        cuts.append(min(n, cuts[-1] + max(1, sizes[k % len(sizes)])))
        k += 1
    return cuts


def fastq_text(rows, id_len=12, seed=0, last_newline=True):
    """FASTQ text of the rows: '@' identifiers of id_len bytes, the symbols, '+', qualities"""
    rows = np.asarray(rows, np.uint8)
    n, L = rows.shape
    rng = np.random.default_rng(seed)
    rec = np.empty((n, id_len + 1 + L + 1 + 2 + L + 1), np.uint8)
    rec[:, 0] = ord("@")
    rec[:, 1:id_len] = rng.integers(ord("a"), ord("z") + 1, size=(n, id_len - 1))
    rec[:, id_len] = 10
    rec[:, id_len + 1: id_len + 1 + L] = rows
    o = id_len + 1 + L
    rec[:, o], rec[:, o + 1], rec[:, o + 2] = 10, ord("+"), 10
    rec[:, o + 3: o + 3 + L] = rng.integers(ord("#"), ord("J"), size=(n, L))
    rec[:, -1] = 10
    t = rec.reshape(-1)
    return t if last_newline or not n else t[:-1]


def feed_rows(v, file, rows, sizes, take=lambda a: a):
    """rows of one file in pieces of `sizes` rows; take: what becomes of a piece before it goes in (e.g. a pinned copy)"""
    cuts = cut_points(rows.shape[0], sizes)
    for a, b in zip(cuts[:-1], cuts[1:]):
        v.add_rows(file, take(np.ascontiguousarray(rows[a:b])))


def feed_fastq(v, text, pair_text, sizes):
    """FASTQ text in pieces of `sizes` bytes (both files cut alike), the unconsumed rest of every piece handed over again
    in front of the next; -> records taken"""
    texts = [np.asarray(text, np.uint8)] + ([] if pair_text is None else [np.asarray(pair_text, np.uint8)])
    at, have, k, total = [0] * len(texts), [0] * len(texts), 0, 0
    while True:
        step = max(1, sizes[k % len(sizes)])
        k += 1
        have = [min(t.size, h + step) for t, h in zip(texts, have)]
        done = [h == t.size for t, h in zip(texts, have)]
        fin = 1 if all(done) else (2 if done[0] else 0) | (4 if len(texts) > 1 and done[1] else 0)
        pieces = [t[a:h] for t, a, h in zip(texts, at, have)]
        used, pused, n = v.add_fastq(pieces[0], pieces[1] if len(pieces) > 1 else None, final=fin)
        at[0] += used
        if len(texts) > 1:
            at[1] += pused
        total += n
        if all(done):
            return total
