"""The pair-order coding of the paired mode that does not preserve the order, restated on the CPU (checker only): the
reference's SeparatedPseudoGenomePersistence::compressReadsOrder (SeparatedPseudoGenomePersistence.cpp:220-339) and
decompressReadsOrder (:341-443) with their serial loops kept literal (the completeOrderInfo remap and the file-flag swaps
included), the parallel form of the encoder that the device runs (vectorised, so that it reaches tens of millions of pairs),
and a generator of orders.

org is the encoder's orgIdxs: org[i] = the original index of entry i of the joined reads lists, a permutation of [0, T);
reads 2q and 2q+1 are mates.  Streams are a dict: the arrays that the form writes under the names of
include/pgrc_decode.h's pgrc_pairorder_streams, plus n_total and form."""
import numpy as np

IGNORE, FILE_FLAGS, COMPLETE, COMPLETE_SINGLE_FILE = 0, 1, 2, 3
FORMS = (IGNORE, FILE_FLAGS, COMPLETE, COMPLETE_SINGLE_FILE)
FORM_NAMES = {IGNORE: "ignore", FILE_FLAGS: "file_flags", COMPLETE: "complete", COMPLETE_SINGLE_FILE: "complete_single_file"}
# (completeOrderInfo, ignorePairOrderInformation, singleFileMode) that each form stands for, as the golden driver passes them
FORM_ARGS = {IGNORE: (False, True, False), FILE_FLAGS: (False, False, False), COMPLETE: (True, False, False),
             COMPLETE_SINGLE_FILE: (True, False, True)}
COMMON = (("off8_flag", np.uint8), ("off_value", np.uint8), ("delta8_flag", np.uint8), ("delta_value", np.int8),
          ("full_offset", np.uint32))
EXTRA = {IGNORE: (), FILE_FLAGS: (("off_base_file_flag", np.uint8), ("nonoff_base_file_flag", np.uint8)),
         COMPLETE: (("pair_base_org_idx", np.uint32),), COMPLETE_SINGLE_FILE: (("rev", np.uint32),)}


def stream_types(form):
    """(name, dtype) of the streams that `form` writes, in the archive's order"""
    return EXTRA[form] if form == COMPLETE_SINGLE_FILE else COMMON + EXTRA[form]


def _pack(form, T, **arrays):
    st = {"n_total": int(T), "form": int(form)}
    for name, dt in stream_types(form):
        st[name] = np.asarray(arrays[name], dtype=dt) if len(arrays[name]) else np.zeros(0, dt)
    return st


def streams_equal(a, b):
    return (int(a["n_total"]) == int(b["n_total"]) and int(a["form"]) == int(b["form"]) and
            all(np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.array_equal(a[k], b[k]) for k, _ in stream_types(int(a["form"]))))


# ---------------------------------------------------------------------------------------------- the literal loops
def compress_literal(org, form):
    """compressReadsOrder (:224-296)"""
    complete, ignore, single = FORM_ARGS[form]
    o = np.asarray(org, np.uint32).tolist()
    T = len(o)
    assert T % 2 == 0
    rev = [0] * T
    for i in range(T):
        rev[o[i]] = i
    if complete and single:
        return _pack(form, T, rev=rev)
    pbo = [0] * (T // 2)
    off_ff, nonoff_ff = [], []
    f8, oval, dfl, dval, full = [], [], [], [], []
    done = bytearray(T)
    ref_prev, prev, match = 0, 0, False
    for i1 in range(T):
        if done[i1]:
            continue
        org_idx = o[i1]
        pair_org_idx = org_idx - 1 if org_idx % 2 else org_idx + 1
        i2 = rev[pair_org_idx]
        done[i2] = 1
        if complete:
            pbo[org_idx // 2] = len(f8) * 2 + org_idx % 2
        rel = i2 - i1
        f8.append(1 if rel <= 255 else 0)
        if rel <= 255:
            oval.append(rel)
            if not complete and not ignore:
                off_ff.append(org_idx % 2)
            continue
        if not complete and not ignore:
            nonoff_ff.append(org_idx % 2)
        delta = rel - ref_prev
        is_delta8 = -128 <= delta <= 127
        dfl.append(1 if is_delta8 else 0)
        if is_delta8:
            match = True
            dval.append(delta)
            ref_prev = rel
        else:
            if not match or ref_prev != prev:
                ref_prev = rel
            full.append(rel)
            match = False
        prev = rel
    return _pack(form, T, off8_flag=f8, off_value=oval, delta8_flag=dfl, delta_value=dval, full_offset=full,
                 pair_base_org_idx=pbo, off_base_file_flag=off_ff, nonoff_base_file_flag=nonoff_ff)


def decompress_literal(st):
    """decompressReadsOrder (:345-442) -> rlIdxOrder as uint32 (with IGNORE: the pairs in base order, the base first)"""
    form = int(st["form"])
    complete, ignore, single = FORM_ARGS[form]
    if single:
        return np.asarray(st["rev"], np.uint32).copy()
    f8 = np.asarray(st["off8_flag"]).tolist()
    oval = np.asarray(st["off_value"]).tolist()
    dfl = np.asarray(st["delta8_flag"]).tolist()
    dval = np.asarray(st["delta_value"]).tolist()
    full = np.asarray(st["full_offset"]).tolist()
    T = len(f8) * 2
    order = [0] * T
    done = bytearray(T)
    pair_offset = 0
    pair_counter = off_idx = del_flag_idx = del_idx = ful_idx = -1
    ref_prev, prev, match = 0, 0, False
    for i in range(T):
        if done[i]:
            continue
        pair_counter += 1
        if f8[pair_counter]:
            off_idx += 1
            pair_offset = oval[off_idx]
        else:
            del_flag_idx += 1
            if dfl[del_flag_idx]:
                del_idx += 1
                pair_offset = ref_prev + dval[del_idx]
                ref_prev = pair_offset
                match = True
                prev = pair_offset
            else:
                ful_idx += 1
                pair_offset = full[ful_idx]
                if not match or ref_prev != prev:
                    ref_prev = pair_offset
                match = False
                prev = pair_offset
        order[pair_counter * 2] = i
        order[pair_counter * 2 + 1] = i + pair_offset
        done[i + pair_offset] = 1
    if complete:
        pbo = np.asarray(st["pair_base_org_idx"]).tolist() + [0] * (T // 2)
        pe = order
        for p in range(T // 2 - 1, -1, -1):
            rl = pbo[p]
            pbo[p * 2] = pe[rl]
            pbo[p * 2 + 1] = pe[rl - 1 if rl % 2 else rl + 1]
        order = pbo
    elif not ignore:
        off_ff = np.asarray(st["off_base_file_flag"]).tolist()
        nonoff_ff = np.asarray(st["nonoff_base_file_flag"]).tolist()
        a = b = -1
        for p in range(T // 2):
            if f8[p]:
                a += 1
                swap = off_ff[a]
            else:
                b += 1
                swap = nonoff_ff[b]
            if swap:
                order[p * 2], order[p * 2 + 1] = order[p * 2 + 1], order[p * 2]
    return np.array(order, dtype=np.uint32)


# ---------------------------------------------------------------------------------------------- the parallel form
# rev[org[i]] = i; mate(i) = rev[org[i] ^ 1]; entry i is a base iff mate(i) > i, and the count of bases before it is its pair
# number.  The far pairs' chain is tests/pairpos_util's three-state form with int8 for int16: before far pair k, refPrev is
# rel[k-1] (state A: pair k-1 was a delta pair; C: a full pair that set refPrev; the start is C with rel[-1] = 0) or rel[k-2]
# (state B: pair k-1 was a full pair that KEPT refPrev).
S_A, S_B, S_C = 0, 1, 2


def _fits8(d):
    return (d >= -128) & (d <= 127)


def chain_states(rel):
    """state before every far pair (rel: int64, far order), by a blocked scan of the state maps: block totals, a serial pass
    over the blocks, a rescan -- what the device's three kernels do"""
    nf = rel.size
    r1 = np.concatenate([np.zeros(1, np.int64), rel[:-1]])[:nf]
    r2 = np.concatenate([np.zeros(2, np.int64), rel[:-2]])[:nf]
    d1, d2 = _fits8(rel - r1), _fits8(rel - r2)
    maps = np.empty((nf, 3), np.uint8)
    maps[:, S_A] = np.where(d1, S_A, S_B)
    maps[:, S_B] = np.where(d2, S_A, S_C)
    maps[:, S_C] = np.where(d1, S_A, S_C)
    block = max(1, int(np.sqrt(nf)))
    nb = (nf + block - 1) // block
    padded = np.tile(np.array([S_A, S_B, S_C], np.uint8), (nb * block, 1))
    padded[:nf] = maps
    m = padded.reshape(nb, block, 3)
    rows = np.arange(nb)
    tot = np.tile(np.array([S_A, S_B, S_C], np.uint8), (nb, 1))
    for j in range(block):
        mj = m[:, j, :]
        tot = np.stack([mj[rows, tot[:, s]] for s in range(3)], axis=1)
    start = np.empty(nb, np.uint8)
    s = S_C
    for b in range(nb):
        start[b] = s
        s = tot[b, s]
    states = np.empty((nb, block), np.uint8)
    cur = start
    for j in range(block):
        states[:, j] = cur
        cur = m[rows, j, cur]
    return states.reshape(-1)[:nf], r1, r2


def compress_parallel(org, form):
    """the encoder as the device runs it (everything vectorised)"""
    org = np.asarray(org, np.uint32)
    T = org.size
    assert T % 2 == 0
    rev = np.empty(T, np.uint32)
    rev[org] = np.arange(T, dtype=np.uint32)
    if form == COMPLETE_SINGLE_FILE:
        return _pack(form, T, rev=rev)
    mate = rev[org ^ np.uint32(1)].astype(np.int64)
    idx = np.arange(T, dtype=np.int64)
    base = np.flatnonzero(mate > idx)
    rel = mate[base] - base
    par = (org[base] & np.uint32(1)).astype(np.uint8)
    near = rel <= 255
    frel = rel[~near]
    st, r1, r2 = chain_states(frel)
    dl = frel - np.where(st == S_B, r2, r1)
    is_delta = _fits8(dl)
    pbo = np.zeros(T // 2, np.uint32)
    if form == COMPLETE:
        pbo[org[base] >> np.uint32(1)] = (2 * np.arange(base.size, dtype=np.int64) + par).astype(np.uint32)
    return _pack(form, T, off8_flag=near, off_value=rel[near], delta8_flag=is_delta, delta_value=dl[is_delta],
                 full_offset=frel[~is_delta], pair_base_org_idx=pbo, off_base_file_flag=par[near],
                 nonoff_base_file_flag=par[~near])


def kinds(st):
    """pairs by kind: near, delta, setting full, keeping full"""
    dfl = np.asarray(st["delta8_flag"]) != 0
    prev_delta = np.concatenate([[False], dfl[:-1]])[:dfl.size]
    return {"near": int((np.asarray(st["off8_flag"]) == 1).sum()), "delta": int(dfl.sum()),
            "full_set": int((~dfl & ~prev_delta).sum()), "full_keep": int((~dfl & prev_delta).sum())}


def boundaries(st):
    """how often the boundary values occur: rel 255 (the last near value) and 256 (the first far one), deltas 127 and -128"""
    full, dv = np.asarray(st["full_offset"]).astype(np.int64), np.asarray(st["delta_value"]).astype(np.int64)
    dfl = np.asarray(st["delta8_flag"]) != 0
    # rel of every far pair: a full pair's is stored; a delta pair's is refPrev + delta -- take it from the literal decoder's walk
    rel_far = np.zeros(dfl.size, np.int64)
    ref_prev = prev = 0
    match = False
    fi = di = 0
    for k in range(dfl.size):
        if dfl[k]:
            r = ref_prev + int(dv[di])
            di += 1
            ref_prev, match = r, True
        else:
            r = int(full[fi])
            fi += 1
            if not match or ref_prev != prev:
                ref_prev = r
            match = False
        prev = r
        rel_far[k] = r
    return {"rel_255": int((np.asarray(st["off_value"]) == 255).sum()), "rel_256": int((rel_far == 256).sum()),
            "delta_127": int((dv == 127).sum()), "delta_m128": int((dv == -128).sum())}


def pairs_are_mates(order, org):
    """every decoded pair (order[2p], order[2p+1]) holds the two entries of one original pair"""
    o = np.asarray(org, np.uint32)[np.asarray(order, np.uint32)]
    return bool(np.array_equal(o[0::2] >> 1, o[1::2] >> 1)) and np.unique(o).size == o.size


# ---------------------------------------------------------------------------------------------- the generator
DEFAULT_MIX = dict(near=0.5, jump=0.15, ret=0.05, special=0.02, drift=40, span=1 << 16)
EXACT_LIMIT = 20000


def _wishes(rng, pairs, near, jump, ret, special, drift, span):
    """per pair: is it near, and the offset it asks for when it is the k-th far pair (drifting from the far pair before,
    jumping to a fresh offset, or returning to the offset two far pairs back)"""
    is_near = rng.random(pairs) < near
    near_val = rng.integers(1, 256, size=pairs, dtype=np.int64)
    is_jump = rng.random(pairs) < jump
    jump_val = rng.integers(256, max(257, span), size=pairs, dtype=np.int64)
    step = rng.integers(-drift, drift + 1, size=pairs, dtype=np.int64)
    is_ret = rng.random(pairs) < ret
    sp = np.where(rng.random(pairs) < special, rng.integers(1, 9, size=pairs), 0)
    return is_near, near_val, is_jump, jump_val, step, is_ret, sp


_SPECIAL_STEPS = (None, None, None, 127, 128, 129, -127, -128, -129)     # sp 1, 2: rel 255 / 256 itself


def make_order(seed, pairs, near=0.5, jump=0.15, ret=0.05, special=0.02, drift=40, span=1 << 16, exact=None, halves=False):
    """org of `pairs` pairs.  The free entries are walked as the decoder walks them; the pair at the next free entry asks for
    an offset: near (1 .. 255) with probability `near`, else far -- a jump to a fresh offset in [256, span) with probability
    `jump`, a return to the offset of the far pair two before with probability `ret`, else a drift by at most `drift` from
    the far pair before (runs of delta pairs when drift <= 127).  `special` of the pairs ask for exactly 255 or 256, or for
    the last far offset +- 127 / 128 / 129.  exact (the default up to EXACT_LIMIT pairs): the mate settles on the free entry
    nearest to the wish, in a serial loop, so that most wishes -- the boundary values among them -- come true as asked.
    Otherwise the order is the sort of keys (base k at k, its mate at k + wish / 2): vectorised for millions of pairs, the
    offsets come out near the wishes and the mix of kinds is kept, but no single value is hit on purpose.  halves (with the
    keys): every mate's key lies behind every base's, so that the first half of the entries are the bases and every offset is
    about `pairs` -- no near pair at all, which the walk cannot give (it runs out of room at the end).  Pair numbers and
    the base's parity are handed out at random."""
    rng = np.random.default_rng(seed)
    T = 2 * pairs
    if exact is None:
        exact = pairs <= EXACT_LIMIT and not halves
    assert not (exact and halves)
    is_near, near_val, is_jump, jump_val, step, is_ret, sp = _wishes(rng, pairs, near, jump, ret, special, drift, span)
    numbers = rng.permutation(pairs).astype(np.int64)
    parity = rng.integers(0, 2, size=pairs, dtype=np.int64)
    org = np.empty(T, np.uint32)
    if not exact:
        k = np.arange(pairs)
        nf_idx = np.flatnonzero(~is_near)
        wish = near_val.copy()
        if nf_idx.size:
            j = is_jump[nf_idx].copy()
            j[0] = True
            s = np.where(j, 0, step[nf_idx])
            walk = np.cumsum(s)
            last = np.maximum.accumulate(np.where(j, np.arange(nf_idx.size), 0))
            far = walk - walk[last] + jump_val[nf_idx][last]
            back = np.flatnonzero(is_ret[nf_idx])
            back = back[back >= 2]
            far[back] = far[back - 2]
            wish[nf_idx] = np.maximum(far, 256)
        keys = np.concatenate([k.astype(np.float64), k + wish / 2.0 + 0.25 * rng.random(pairs) + (pairs + 128 if halves else 0)])
        entry = np.argsort(keys, kind="stable")          # entry -> read (k: the base of pair k, pairs + k: its mate)
        is_mate = entry >= pairs
        pk = np.where(is_mate, entry - pairs, entry)
        org[:] = (2 * numbers[pk] + (parity[pk] ^ is_mate)).astype(np.uint32)
        return org
    free = bytearray([1]) * T
    i = 0
    far_hist = [0, 0]           # the offsets of the last two far pairs
    for k in range(pairs):
        while not free[i]:
            i += 1
        free[i] = 0
        room = T - 1 - i
        if sp[k] in (1, 2):
            wish = 254 + int(sp[k])
        elif sp[k]:
            wish = far_hist[1] + _SPECIAL_STEPS[sp[k]]
        elif is_near[k]:
            wish = int(near_val[k])
        elif is_jump[k]:
            wish = int(jump_val[k])
        elif is_ret[k]:
            wish = far_hist[0] + int(step[k]) // 8
        else:
            wish = far_hist[1] + int(step[k])
        wish = min(max(wish, 1), room)
        t = i + wish
        s = 0
        while True:             # the nearest free entry after i
            if t + s < T and free[t + s]:
                t += s
                break
            if t - s > i and free[t - s]:
                t -= s
                break
            s += 1
        free[t] = 0
        if t - i > 255:
            far_hist = [far_hist[1], t - i]
        q, b = int(numbers[k]), int(parity[k])
        org[i] = 2 * q + b
        org[t] = 2 * q + (1 - b)
    return org


def split_three(org, seed):
    """org cut into three uneven parts, one of them empty (which one depends on seed)"""
    org = np.asarray(org, np.uint32)
    rng = np.random.default_rng(seed)
    cut = int(rng.integers(0, org.size + 1)) if org.size else 0
    cut = min(cut, org.size // 3) if seed % 2 else cut
    parts = [org[:cut], org[cut:]]
    parts.insert(seed % 3, org[:0])
    return parts
