"""The pair-order decoder as the device runs it, restated in numpy and plain Python (checker only): pgrc_pairorder_decode of
include/pgrc_decode.h, pgrc_amd/csrc/pairorder.hip, DESIGN.md 4.11.

  offsets   every pair's offset from flag scans (cumulative sums) and one segmented sum over the pairs: a delta pair ADDs its
            int8, a full pair SETs its value unless the far pair before it was a delta pair (then it adds nothing), a near
            pair adds nothing
  land      the landing, literally: the slots in words of 64 with the word relaxation (M = E; M' = E | the marks of the open
            lanes that fall into the word; M' == M ends it; else M = E | the marks of the open lanes below the first bit that
            changed: those lanes are final bases), marks
            beyond the word in a bit ring of 4 batches or, from 3 batches on, in a bitmap that is merged into the ring batch by
            batch.  The batch size is a parameter, so that a test reaches the bitmap with a few hundred slots.
  tails     FILE_FLAGS: the predicated swap; COMPLETE: the gather
  checks    every refusal of the header raises Refused with the device's wording

Streams are dicts as tests/pairorder_util.py makes them; the counts n_off8, n_delta_flag, n_delta8, n_full are the arrays'
sizes unless the dict names them."""
import numpy as np

import pairorder_util as po

BATCH = 16384           # PGRC_PAIRORDER_DECODE_BATCH
FULL = (1 << 64) - 1


class Refused(Exception):
    """PGRC_E_PARAM of pgrc_pairorder_decode; str(e) is part of the device's message"""


def _count(st, name, stream):
    return int(st.get(name, 0 if st.get(stream) is None else np.asarray(st[stream]).size))


def check_streams(st):
    """the checks that need no device (pgrc_pairorder_check_streams) -> (form, T, P, counts)"""
    form, T = int(st["form"]), int(st["n_total"])
    if form not in po.FORMS:
        raise Refused("unknown form")
    if T >= 1 << 32:
        raise Refused("2^32 entries or more")
    if T & 1:
        raise Refused("n_total is odd")
    P = T // 2
    if form == po.COMPLETE_SINGLE_FILE:
        if T and st.get("rev") is None:
            raise Refused("rev is absent")
        return form, T, P, None
    n = {k: _count(st, k, s) for k, s in (("n_off8", "off_value"), ("n_delta_flag", "delta8_flag"), ("n_delta8", "delta_value"),
                                          ("n_full", "full_offset"))}
    for cnt, name in ((P, "off8_flag"), (n["n_off8"], "off_value"), (n["n_delta_flag"], "delta8_flag"),
                      (n["n_delta8"], "delta_value"), (n["n_full"], "full_offset")):
        if cnt and (st.get(name) is None or np.asarray(st[name]).size == 0):
            raise Refused(name + " is NULL with a non-zero count")
    if form == po.COMPLETE and P and st.get("pair_base_org_idx") is None:
        raise Refused("pair_base_org_idx is absent")
    if form == po.FILE_FLAGS and ((n["n_off8"] and st.get("off_base_file_flag") is None) or
                                  (n["n_delta_flag"] and st.get("nonoff_base_file_flag") is None)):
        raise Refused("off_base_file_flag or nonoff_base_file_flag is absent")
    if max(n.values()) > P:
        raise Refused("a stream holds more elements than there are pairs")
    return form, T, P, n


def offsets(st):
    """-> (d: int64[P], the offsets as decoded -- not yet held to any range; near: bool[P]; kinds (near, delta, full))"""
    form, T, P, n = check_streams(st)
    f8 = np.asarray(st["off8_flag"], np.uint8)[:P] != 0 if P else np.zeros(0, bool)
    near_inc = np.cumsum(f8)
    n_near = int(near_inc[-1]) if P else 0
    if n_near != n["n_off8"]:
        raise Refused("off8_flag holds %d near pairs, n_off8 is %d" % (n_near, n["n_off8"]))
    nf = P - n_near
    if nf != n["n_delta_flag"]:
        raise Refused("off8_flag holds %d far pairs, n_delta_flag is %d" % (nf, n["n_delta_flag"]))
    dfl = np.asarray(st["delta8_flag"], np.uint8)[:nf] != 0 if nf else np.zeros(0, bool)
    del_inc = np.cumsum(dfl)
    n_del = int(del_inc[-1]) if nf else 0
    if n_del != n["n_delta8"]:
        raise Refused("delta8_flag holds %d delta pairs, n_delta8 is %d" % (n_del, n["n_delta8"]))
    if nf - n_del != n["n_full"]:
        raise Refused("delta8_flag holds %d full pairs, n_full is %d" % (nf - n_del, n["n_full"]))
    # the chain over the far pairs: (value, set)
    val = np.zeros(nf, np.int64)
    if n_del:
        val[dfl] = np.asarray(st["delta_value"], np.int8)[:n_del].astype(np.int64)
    full = np.asarray(st["full_offset"], np.uint32)[:nf - n_del].astype(np.int64) if nf - n_del else np.zeros(0, np.int64)
    prev_delta = np.concatenate([[False], dfl[:-1]])[:nf]
    sets = ~dfl & ~prev_delta
    full_at = np.zeros(nf, np.int64)
    full_at[~dfl] = full
    val[sets] = full_at[sets]                 # (a keeping full pair adds 0)
    # the segmented inclusive sum: the running sum since -- and with -- the last SET
    cs = np.cumsum(val)
    last = np.maximum.accumulate(np.where(sets, np.arange(nf), -1)) if nf else np.zeros(0, np.int64)
    ref = np.where(last >= 0, cs - cs[np.maximum(last, 0)] + val[np.maximum(last, 0)], cs)
    far_d = np.where(dfl, ref, full_at)
    d = np.zeros(P, np.int64)
    if n_near:
        d[f8] = np.asarray(st["off_value"], np.uint8)[:n_near].astype(np.int64)
    d[~f8] = far_d
    return d, f8, (n_near, n_del, nf - n_del)


def settle(E, k, d, P):
    """one word: -> (M, rounds, the open lanes' (lane, pair, offset)) or None when 64 rounds do not settle it.  d: the offsets
    as the device holds them (0 = below 1)"""
    M = E
    for r in range(1, 65):
        lanes, Mn, rank, src = [], E, 0, [64] * 64          # src: the lowest lane that marks a slot
        for j in range(64):
            if (M >> j) & 1:
                continue
            kk = k + rank
            rank += 1
            dd = int(d[kk]) if kk < P else 0
            lanes.append((j, kk, dd))
            if dd and j + dd < 64:
                Mn |= 1 << (j + dd)
                src[j + dd] = min(src[j + dd], j)
        if Mn == M:
            return M, r, lanes
        x = ((Mn ^ M) & -(Mn ^ M)).bit_length() - 1          # the first bit that changed: M is final below it
        M = E | sum(1 << t for t in range(64) if src[t] < x)
    return None


def land(d, T, batch=BATCH):
    """-> (pe: uint32[T], findings: set of names, words, rounds).  After a finding pe is not to be used."""
    assert batch % 64 == 0 and T % 2 == 0
    P = T // 2
    d = np.minimum(np.where(np.asarray(d, np.int64) < 1, 0, d), 0xFFFFFFFF)
    findings = set()
    if P and (d == 0).any():
        findings.add("a decoded offset below 1")
    bw = batch // 64                                    # words of a batch
    ring = [0] * (4 * bw)
    nbatch = (T + batch - 1) // batch
    gmark = [0] * (max(nbatch, 1) * bw)
    pe = np.zeros(T, np.uint32)
    k = words = rounds = 0
    for w in range((T + 63) // 64):
        if k >= P:
            break
        if w % bw == 0:                                 # entering batch m
            m = w // bw
            for i in range(bw):
                ring[(m & 3) * bw + i] |= gmark[m * bw + i]
                ring[((m + 3) & 3) * bw + i] = 0
        slot0 = w * 64
        E = ring[w % (4 * bw)]
        if T - slot0 < 64:
            E |= (FULL << (T - slot0)) & FULL
        got = settle(E, k, d, P)
        if got is None:
            findings.add("did not settle")
            return pe, findings, words, rounds
        M, r, lanes = got
        rounds += r
        words += 1
        for j, kk, dd in lanes:
            slot, mate = slot0 + j, slot0 + j + dd
            if kk >= P:
                findings.add("an entry that no pair takes")
            elif dd == 0:
                findings.add("a decoded offset below 1")
            elif mate >= T:
                findings.add("a mate beyond the last entry")
            else:
                pe[2 * kk], pe[2 * kk + 1] = slot, mate
                if j + dd >= 64:
                    if dd < 3 * batch:
                        ring[(mate // 64) % (4 * bw)] |= 1 << (mate % 64)
                    else:
                        gmark[mate // 64] |= 1 << (mate % 64)
        k = min(k + len(lanes), P)
    if k < P:
        findings.add("the entries run out before the pairs do")
    return pe, findings, words, rounds


def is_base_ordered_permutation(pe):
    """the device's check of the landed array: every entry once, the bases ascend, every mate after its base"""
    pe = np.asarray(pe, np.int64)
    T = pe.size
    seen = np.zeros(T, bool)
    ok = (pe[1::2] > pe[0::2]) & (pe[1::2] < T)
    ok[1:] &= pe[2::2] > pe[0:-2:2]
    if not ok.all():
        return False
    seen[pe] = True
    return bool(seen.all())


def decode(st, batch=BATCH, stats=None):
    """pgrc_pairorder_decode -> rlIdxOrder (uint32), or raises Refused.  stats: a dict that receives landing_words,
    landing_rounds and the pairs by kind"""
    form, T, P, _ = check_streams(st)
    if form == po.COMPLETE_SINGLE_FILE:
        return np.asarray(st["rev"], np.uint32)[:T].copy()
    d, near, kinds = offsets(st)
    pe, findings, words, rounds = land(d, T, batch)
    if findings:
        raise Refused("; ".join(sorted(findings)))
    if not is_base_ordered_permutation(pe):
        raise Refused("the landed pairs are not a permutation of the entries")
    if stats is not None:
        stats.update(landing_words=words, landing_rounds=rounds, n_near=kinds[0], n_delta=kinds[1], n_full=kinds[2])
    if form == po.IGNORE:
        return pe
    if form == po.FILE_FLAGS:
        flag = np.zeros(P, bool)
        flag[near] = np.asarray(st["off_base_file_flag"], np.uint8)[:kinds[0]] != 0
        flag[~near] = np.asarray(st["nonoff_base_file_flag"], np.uint8)[:P - kinds[0]] != 0
        out = pe.copy()
        out[0::2] = np.where(flag, pe[1::2], pe[0::2])
        out[1::2] = np.where(flag, pe[0::2], pe[1::2])
        return out
    r = np.asarray(st["pair_base_org_idx"], np.uint32)[:P].astype(np.int64)
    if (r >= T).any():
        raise Refused("a pair_base_org_idx value of n_total or more")
    out = np.empty(T, np.uint32)
    out[0::2] = pe[r]
    out[1::2] = pe[r ^ 1]
    return out


# ---------------------------------------------------------------------------------------------- orders with chosen offsets
def order_from_pairs(pairs_of_slots, T, seed=0):
    """org for a given landing: pairs_of_slots lists (base slot, mate slot) in any order; pair numbers and the base's parity
    are handed out at random"""
    rng = np.random.default_rng(seed)
    ps = sorted(pairs_of_slots)
    assert len(ps) * 2 == T and sorted(s for p in ps for s in p) == list(range(T))
    numbers, parity = rng.permutation(len(ps)), rng.integers(0, 2, size=len(ps))
    org = np.empty(T, np.uint32)
    for q, (b, m) in enumerate(ps):
        assert b < m
        org[b] = 2 * numbers[q] + parity[q]
        org[m] = 2 * numbers[q] + (1 - parity[q])
    return org


def order_with_offsets(wishes, pairs, seed=0):
    """an order of `pairs` pairs in which the given offsets occur: the free slots are walked as the decoder walks them, and the
    pair at the next free slot takes the next wish that still fits (its mate free and inside), else the nearest free slot"""
    T = 2 * pairs
    free = bytearray([1]) * T
    todo = list(wishes)
    out, i = [], 0
    for _ in range(pairs):
        while not free[i]:
            i += 1
        free[i] = 0
        t = None
        for n, w in enumerate(todo):
            if i + w < T and free[i + w]:
                t = i + todo.pop(n)
                break
        if t is None:
            t = i + 1
            while not free[t]:
                t += 1
        free[t] = 0
        out.append((i, t))
    assert not todo, todo
    return order_from_pairs(out, T, seed)


def adjacent_order(pairs, seed=0):
    """d = 1 everywhere"""
    return order_from_pairs([(2 * q, 2 * q + 1) for q in range(pairs)], 2 * pairs, seed)


def nested_order(pairs, seed=0):
    """mate = T - 1 - base"""
    return order_from_pairs([(q, 2 * pairs - 1 - q) for q in range(pairs)], 2 * pairs, seed)


def constant_offset_order(dd, blocks, seed=0):
    """every offset is exactly dd: blocks of 2 * dd slots, the first dd of each the bases"""
    return order_from_pairs([(2 * dd * b + q, 2 * dd * b + q + dd) for b in range(blocks) for q in range(dd)], 2 * dd * blocks, seed)


def spread_offsets_order(wishes, pairs, every, seed=0):
    """order_with_offsets with the wishes handed out one at a time, to every `every`-th pair (the pairs between them are
    neighbours), so that their bases lie in different words and batches"""
    T = 2 * pairs
    free = bytearray([1]) * T
    todo = list(wishes)
    out, i = [], 0
    for q in range(pairs):
        while not free[i]:
            i += 1
        free[i] = 0
        t = None
        if q % every == 0:
            for n, w in enumerate(todo):
                if i + w < T and free[i + w]:
                    t = i + todo.pop(n)
                    break
        if t is None:
            t = i + 1
            while not free[t]:
                t += 1
        free[t] = 0
        out.append((i, t))
    assert not todo, todo
    return order_from_pairs(out, T, seed)


def batch_wishes(batch):
    """offsets around the ring's reach (3 batches) and beyond it, and around a word and a batch"""
    return [4 * batch + 5, 3 * batch + 1, 3 * batch, 3 * batch - 1, 2 * batch + 1, batch, batch - 1, 65, 64, 63,
            4 * batch + 5, 3 * batch + 1, 3 * batch, 3 * batch - 1]


def generated_orders(batch=BATCH):
    """(name, org) of the orders the decoder is held to: the generator at sizes around a word, the all-adjacent order,
    constant offsets around a word and around the near / far limit, the nested order, the halves order, and one order with
    offsets around the reach of the ring of `batch`-slot batches"""
    out = [("make_order_%d" % p, po.make_order(4100 + p, p)) for p in (1, 2, 31, 32, 33, 63, 64, 65, 2400)]
    out.append(("adjacent", adjacent_order(256, 1)))
    out += [("offset_%d" % dd, constant_offset_order(dd, 3, dd)) for dd in (63, 64, 65, 255, 256)]
    out.append(("nested", nested_order(300, 2)))
    out.append(("halves", po.make_order(77, 500, halves=True)))
    out.append(("batches", spread_offsets_order(batch_wishes(batch), 6 * batch, max(1, batch // 4) + 1, 3)))
    return out


def near_streams(offs, form=po.IGNORE, **more):
    """streams of near pairs alone with the given offsets (by hand: they need not describe any order)"""
    n = len(offs)
    st = {"n_total": 2 * n, "form": form, "off8_flag": np.ones(n, np.uint8), "off_value": np.asarray(offs, np.uint8),
          "delta8_flag": np.zeros(0, np.uint8), "delta_value": np.zeros(0, np.int8), "full_offset": np.zeros(0, np.uint32)}
    st.update(more)
    return st


def refusal_cases():
    """(name, streams, a part of the message) of every refusal of pgrc_pairorder_decode; a stream that is None is NULL"""
    org = po.make_order(31, 3000)
    ff, co, sf = (po.compress_literal(org, f) for f in (po.FILE_FLAGS, po.COMPLETE, po.COMPLETE_SINGLE_FILE))
    n = {"n_off8": ff["off_value"].size, "n_delta_flag": ff["delta8_flag"].size, "n_delta8": ff["delta_value"].size,
         "n_full": ff["full_offset"].size}
    assert min(n.values()) > 2
    far = lambda flags, vals, full: {"n_total": 2 * len(flags), "form": po.IGNORE, "off8_flag": np.zeros(len(flags), np.uint8),     # noqa: E731
                                     "off_value": np.zeros(0, np.uint8), "delta8_flag": np.asarray(flags, np.uint8),
                                     "delta_value": np.asarray(vals, np.int8), "full_offset": np.asarray(full, np.uint32)}
    zero_off = dict(ff, off_value=ff["off_value"].copy())
    zero_off["off_value"][5] = 0
    high_pbo = dict(co, pair_base_org_idx=co["pair_base_org_idx"].copy())
    high_pbo["pair_base_org_idx"][17] = org.size
    return [
        ("odd n_total", dict(ff, n_total=org.size - 1), "odd"),
        ("2^32 entries", dict(ff, n_total=1 << 32), "2^32"),
        ("unknown form", dict(ff, form=4), "form"),
        ("negative form", dict(ff, form=-1), "form"),
        ("NULL off8_flag", dict(ff, off8_flag=None), "off8_flag is NULL"),
        ("NULL off_value", dict(ff, off_value=None, **n), "off_value is NULL"),
        ("NULL delta8_flag", dict(ff, delta8_flag=None, **n), "delta8_flag is NULL"),
        ("NULL delta_value", dict(ff, delta_value=None, **n), "delta_value is NULL"),
        ("NULL full_offset", dict(ff, full_offset=None, **n), "full_offset is NULL"),
        ("COMPLETE without pair_base_org_idx", dict(co, pair_base_org_idx=None), "pair_base_org_idx is absent"),
        ("FILE_FLAGS without the near flags", dict(ff, off_base_file_flag=None), "is absent"),
        ("FILE_FLAGS without the far flags", dict(ff, nonoff_base_file_flag=None), "is absent"),
        ("COMPLETE_SINGLE_FILE without rev", dict(sf, rev=None), "rev is absent"),
        ("near flags != n_off8", dict(ff, **dict(n, n_off8=n["n_off8"] - 1)), "n_off8 is"),
        ("far flags != n_delta_flag", dict(ff, **dict(n, n_delta_flag=n["n_delta_flag"] - 1)), "n_delta_flag is"),
        ("delta flags != n_delta8", dict(ff, **dict(n, n_delta8=n["n_delta8"] - 1)), "n_delta8 is"),
        ("full flags != n_full", dict(ff, **dict(n, n_full=n["n_full"] - 1)), "n_full is"),
        ("a near offset of 0", zero_off, "offset below 1"),
        ("a delta chain that reaches 0", far([0, 1, 1], [-3, -2], [5]), "offset below 1"),
        ("a delta chain below 0", far([1, 1], [-1, 1], []), "offset below 1"),
        ("a mate beyond the end", near_streams([1, 1, 2]), "mate beyond"),
        ("a full offset of 2^32 - 1", far([0, 0], [], [1, 0xFFFFFFFF]), "mate beyond"),
        ("a delta chain above 2^32", far([0, 1, 1], [127, 127], [0xFFFFFFF0]), "mate beyond"),
        ("two pairs on one entry, same word", near_streams([2, 1]), "no pair takes"),
        ("two pairs on one entry, the gap a word later", near_streams([2, 1] + [1] * 31), "not a permutation"),
        ("pair_base_org_idx >= T", high_pbo, "pair_base_org_idx value"),
    ]
