"""The pair-position coding of the order-preserving paired mode, restated on the CPU (checker only): the reference's
SeparatedPseudoGenomePersistence::compressReadsPgPositions (SeparatedPseudoGenomePersistence.cpp:445-574) and
decompressReadsPgPositions (:582-673) with their serial loops kept literal, the three-state form of the encoder's chain
that the device runs (vectorised, so that it reaches tens of millions of pairs), and a generator of position arrays.

Layouts: the encoder takes orgIdx2PgPos with the mates INTERLEAVED ([2p] the base read of pair p, [2p+1] its mate); the
decoder returns pgPos FILE-MAJOR ([p] the base, [P + p] the mate).  Streams are a dict: the eight arrays by the names of
include/pgrc_decode.h's pgrc_pairpos_streams, plus n_total and pos_width."""
import numpy as np

STREAMS = ("base_pos", "off16_flag", "off_base_first", "off_value", "delta16_flag", "delta_base_first", "delta_value",
           "not_base_pos")
M64 = (1 << 64) - 1


def pos_dtype(W):
    return np.uint64 if W == 8 else np.uint32


def _i64(x):
    """a value stored into an int64_t"""
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def interleaved(file_major):
    fm = np.asarray(file_major, np.uint64)
    P = fm.size // 2
    out = np.empty(2 * P, np.uint64)
    out[0::2], out[1::2] = fm[:P], fm[P:]
    return out


def file_major(org):
    org = np.asarray(org, np.uint64)
    return np.concatenate([org[0::2], org[1::2]])


def _pack(W, T, base, f16, obf, oval, dfl, dbf, dval, nbp):
    return {"n_total": int(T), "pos_width": int(W), "base_pos": np.asarray(base, np.uint64).astype(pos_dtype(W)),
            "off16_flag": np.asarray(f16, np.uint8), "off_base_first": np.asarray(obf, np.uint8),
            "off_value": np.asarray(oval, np.uint16), "delta16_flag": np.asarray(dfl, np.uint8),
            "delta_base_first": np.asarray(dbf, np.uint8), "delta_value": np.asarray(dval, np.int16),
            "not_base_pos": np.asarray(nbp, np.uint64).astype(pos_dtype(W))}


# ---------------------------------------------------------------------------------------------- the literal loops
def compress_literal(org, W):
    """compressReadsPgPositions<uint_pg_len> (:464-530), not singleFileMode, deltaPairEncodingEnabled"""
    org_np = np.asarray(org, np.uint64)
    T = org_np.size
    assert T % 2 == 0
    wmask = (1 << (8 * W)) - 1
    pairs = T // 2
    base_pos = org_np[0::2].copy()
    bpp_rank = np.argsort(base_pos, kind="stable").tolist()         # stable_sort of the pair numbers by basePairPos
    o = org_np.tolist()
    f16, obf, oval, dfl, dbf, dval, nbp = [], [], [], [], [], [], []
    ref_prev, prev, match = 0, 0, False
    for p in range(pairs):
        i = bpp_rank[p] * 2
        is_base_before = o[i] < o[i + 1]
        rel = ((o[i + 1] - o[i]) if is_base_before else (o[i] - o[i + 1])) & wmask
        is16 = rel <= 0xFFFF
        f16.append(1 if is16 else 0)
        if is16:
            obf.append(1 if is_base_before else 0)
            oval.append(rel)
            continue
        delta = _i64(rel - ref_prev)
        is_delta16 = -32768 <= delta <= 32767
        dfl.append(1 if is_delta16 else 0)
        if is_delta16:
            match = True
            dbf.append(1 if is_base_before else 0)
            dval.append(delta)
            ref_prev = rel
        else:
            if not match or ref_prev != prev:
                ref_prev = rel
            nbp.append(o[i + 1] & wmask)
            match = False
        prev = rel
    return _pack(W, T, base_pos, f16, obf, oval, dfl, dbf, dval, nbp)


def decompress_literal(st):
    """decompressReadsPgPositions<uint_pg_len> (:627-671) -> pgPos as uint64, file-major"""
    W, T = int(st["pos_width"]), int(st["n_total"])
    wmask = (1 << (8 * W)) - 1
    pairs = T // 2
    base = np.asarray(st["base_pos"], np.uint64)
    assert base.size == pairs
    bpp_rank = np.argsort(base, kind="stable").tolist()
    pg = base.tolist() + [0] * pairs
    f16 = np.asarray(st["off16_flag"]).tolist()
    obf, oval = np.asarray(st["off_base_first"]).tolist(), np.asarray(st["off_value"]).tolist()
    dfl = np.asarray(st["delta16_flag"]).tolist()
    dbf, dval = np.asarray(st["delta_base_first"]).tolist(), np.asarray(st["delta_value"]).tolist()
    nbp = np.asarray(st["not_base_pos"]).tolist()
    off_idx = del_flag_idx = del_idx = nbp_idx = -1
    ref_prev, prev, match = 0, 0, False
    for i in range(pairs):
        p = bpp_rank[i]
        if f16[i] == 1:
            off_idx += 1
            delta = oval[off_idx]
            if obf[off_idx] == 0:
                delta = -delta
            nbp_pos = pg[p] + delta
        else:
            del_flag_idx += 1
            if dfl[del_flag_idx]:
                del_idx += 1
                delta = ref_prev + dval[del_idx]
                ref_prev = delta
                prev = delta
                if dbf[del_idx] == 0:
                    delta = -delta
                nbp_pos = pg[p] + delta
                match = True
            else:
                nbp_idx += 1
                nbp_pos = nbp[nbp_idx]
                delta = _i64(nbp_pos - pg[p])
                if delta < 0:
                    delta = -delta
                if not match or ref_prev != prev:
                    ref_prev = delta
                match = False
                prev = delta
        pg[pairs + p] = nbp_pos & wmask
    return np.array(pg, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------- the three-state form
# Before far pair k, refPrev is rel[k-1] (state A: pair k-1 was a delta pair; C: a full pair that set refPrev; the chain
# starts in C with rel[-1] = 0) or rel[k-2] (state B: pair k-1 was a full pair that KEPT refPrev, i.e. came right after a
# delta pair).  Pair k maps A -> (d1 ? A : B), B -> (d2 ? A : C), C -> (d1 ? A : C), with d1 = "rel[k] - rel[k-1] fits
# int16" and d2 the same against rel[k-2].  Maps compose associatively; the state before k is the composition of the
# maps before k applied to C.
S_A, S_B, S_C = 0, 1, 2


def _fits16(d_u64):
    d = d_u64.view(np.int64)
    return (d >= -32768) & (d <= 32767)


def chain_states(rel):
    """state before every far pair (rel: uint64, far order), by a blocked scan of the maps: block totals, a serial pass
    over the blocks, a rescan -- what the device's three kernels do"""
    nf = rel.size
    r1 = np.concatenate([np.zeros(1, np.uint64), rel[:-1]])[:nf]
    r2 = np.concatenate([np.zeros(2, np.uint64), rel[:-2]])[:nf]
    d1, d2 = _fits16(rel - r1), _fits16(rel - r2)
    maps = np.empty((nf, 3), np.uint8)
    maps[:, S_A] = np.where(d1, S_A, S_B)
    maps[:, S_B] = np.where(d2, S_A, S_C)
    maps[:, S_C] = np.where(d1, S_A, S_C)
    _BLOCK = max(1, int(np.sqrt(nf)))
    nb = (nf + _BLOCK - 1) // _BLOCK
    padded = np.tile(np.array([S_A, S_B, S_C], np.uint8), (nb * _BLOCK, 1))
    padded[:nf] = maps
    m = padded.reshape(nb, _BLOCK, 3)
    rows = np.arange(nb)
    tot = np.tile(np.array([S_A, S_B, S_C], np.uint8), (nb, 1))          # per block: the composition of its maps
    for j in range(_BLOCK):
        mj = m[:, j, :]
        tot = np.stack([mj[rows, tot[:, s]] for s in range(3)], axis=1)
    start = np.empty(nb, np.uint8)
    s = S_C
    for b in range(nb):
        start[b] = s
        s = tot[b, s]
    states = np.empty((nb, _BLOCK), np.uint8)
    cur = start
    for j in range(_BLOCK):
        states[:, j] = cur
        cur = m[rows, j, cur]
    return states.reshape(-1)[:nf], r1, r2


def compress_states(org, W):
    """the encoder with the chain as a scan of state maps (everything vectorised)"""
    org = np.asarray(org, np.uint64)
    T = org.size
    assert T % 2 == 0
    wmask = np.uint64((1 << (8 * W)) - 1)
    base, mate = org[0::2], org[1::2]
    rank = np.argsort(base, kind="stable")
    b, m = base[rank], mate[rank]
    first = b < m
    rel = np.where(first, m - b, b - m) & wmask
    near = rel <= 0xFFFF
    far = ~near
    frel, fm, ffirst = rel[far], m[far], first[far]
    st, r1, r2 = chain_states(frel)
    ref = np.where(st == S_B, r2, r1)
    dl = frel - ref
    is_delta = _fits16(dl)
    return _pack(W, T, base, near, first[near], rel[near], is_delta, ffirst[is_delta], dl.view(np.int64)[is_delta],
                 fm[~is_delta] & wmask)


def kinds(st):
    """pairs by kind: near, delta, setting full, keeping full"""
    dfl = np.asarray(st["delta16_flag"]) != 0
    prev_delta = np.concatenate([[False], dfl[:-1]])[:dfl.size]
    return {"near": int((np.asarray(st["off16_flag"]) == 1).sum()), "delta": int(dfl.sum()),
            "full_set": int((~dfl & ~prev_delta).sum()), "full_keep": int((~dfl & prev_delta).sum())}


def ties(org):
    base = np.sort(np.asarray(org, np.uint64)[0::2])
    return int((base[1:] == base[:-1]).sum())


def streams_equal(a, b):
    return (int(a["n_total"]) == int(b["n_total"]) and int(a["pos_width"]) == int(b["pos_width"]) and
            all(np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.array_equal(a[k], b[k]) for k in STREAMS))


# ---------------------------------------------------------------------------------------------- the generator
DEFAULT_MIX = dict(near=0.5, jump=0.15, ret=0.05, tie=0.02, special=0.02, drift=2000, hi=True)


def make_positions(seed, pairs, W, near=0.5, jump=0.15, ret=0.05, tie=0.02, special=0.02, drift=2000, hi=True, top=None):
    """orgIdx2PgPos (interleaved) of `pairs` pairs.  In rank order a pair is near with probability `near` (rel uniform
    in [0, 65535]; `special` of them exactly 0 -- mate == base -- or 65535); the others form the chain: a far pair is a
    jump to a fresh rel with probability `jump` (isolated far pairs; `special` of them exactly 65536), else it drifts by
    at most `drift` from the far pair before (runs of delta pairs; `special` of the steps are exactly 32767, 32768,
    -32768 or -32769), and `ret` of the far pairs return to the rel of the pair two before (delta -> full -> delta when
    that follows a jump after a drift; delta -> full -> full comes from two jumps).  `tie` of the pairs share their
    base position with another pair.  W = 8 with `hi`: base positions up to 2^36, most above 2^32; `top`: every
    position at most `top` (at least 2^30) instead."""
    rng = np.random.default_rng(seed)
    if top is None:
        top = (1 << 36) if (W == 8 and hi) else (1 << 32) - 1
    assert top >= 1 << 30
    base = rng.integers(0, top, size=pairs, dtype=np.uint64)
    if pairs > 1:
        t = np.flatnonzero(rng.random(pairs) < tie)
        base[t] = base[rng.integers(0, pairs, size=t.size)]
    rank = np.argsort(base, kind="stable")
    is_near = rng.random(pairs) < near
    rel = rng.integers(0, 65536, size=pairs, dtype=np.int64)
    sp = rng.random(pairs) < special
    rel[sp] = rng.choice(np.array([0, 65535]), size=int(sp.sum()))
    nf = int((~is_near).sum())
    if nf:
        is_jump = rng.random(nf) < jump
        is_jump[0] = True
        jump_val = rng.integers(1 << 18, 1 << 28, size=nf, dtype=np.int64)
        jump_val[rng.random(nf) < special] = 65536
        step = rng.integers(-drift, drift + 1, size=nf, dtype=np.int64)
        sps = rng.random(nf) < special
        step[sps] = rng.choice(np.array([32767, 32768, -32768, -32769]), size=int(sps.sum()))
        step[is_jump] = 0
        walk = np.cumsum(step)
        last = np.maximum.accumulate(np.where(is_jump, np.arange(nf), 0))
        frel = walk - walk[last] + jump_val[last]
        back = np.flatnonzero(rng.random(nf) < ret)
        back = back[back >= 2]
        frel[back] = frel[back - 2] + rng.integers(-drift, drift + 1, size=back.size)
        frel = np.clip(frel, 65536, (1 << 29))
        rel[~is_near] = frel
    rel_u = rel.astype(np.uint64)
    b = base[rank]
    first = rng.random(pairs) < 0.5
    first = np.where(b < rel_u, True, first)                # the mate stays inside [0, top]
    first = np.where(b + rel_u > np.uint64(top), False, first)
    first &= rel_u != 0
    mate_r = np.where(first, b + rel_u, b - rel_u)
    org = np.empty(2 * pairs, np.uint64)
    org[0::2] = base
    org[2 * rank + 1] = mate_r
    return org
