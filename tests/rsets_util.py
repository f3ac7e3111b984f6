"""The four edits of DividedPCLReadsSets (readsset/DividedPCLReadsSets.cpp:145-246) restated twice, for the tests of
include/pgrc_readsets.h: the reference's loops line by line (`literal_*`: the backward walk of the move with its unsigned
counters, the early end once hqCounter is 0, the ignoreLqSet / ignoreNSet underflows), and the form the device uses, one class
per original index (`class_*`).  A state is a dict: A (readsTotalCount), hq / lq / n (uint8 [rows, row bytes]; n is None
without an N set), lq_map / n_map (uint32, the guard A last; n_map is None without an N set)."""
import os

import numpy as np

M32 = 0xFFFFFFFF
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def row_bytes(L, symbols):
    return (L + 3) // 4 if symbols == 4 else (L + 2) // 3 if symbols == 5 else 0


def set_shapes(L, separate_n, n_reads_lq=False):
    """(symbols, row bytes) of the HQ, LQ and N set (DividedPCLReadsSets.cpp:10-21)"""
    sym = (4 if (separate_n or n_reads_lq) else 5, 4 if separate_n else 5, 5 if separate_n else 0)
    return sym, tuple(row_bytes(L, s) for s in sym)


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def random_state(rng, L, separate_n, A, p_lq=0.3, p_n=0.15, n_reads_lq=False):
    """a valid state of A reads: every read in one set, rows of random packed bytes (the edits never look inside a row)"""
    sym, rb = set_shapes(L, separate_n, n_reads_lq)
    u = rng.random(A)
    cls = np.where(u < p_lq, 1, np.where((u < p_lq + p_n) & bool(separate_n), 2, 0)).astype(np.uint8)
    rows = [rng.integers(0, 125 if sym[k] == 5 else 256, size=(int((cls == k).sum()), rb[k]), dtype=np.uint8) for k in range(3)]
    lq_map = np.concatenate([np.flatnonzero(cls == 1), [A]]).astype(np.uint32)
    n_map = np.concatenate([np.flatnonzero(cls == 2), [A]]).astype(np.uint32) if separate_n else None
    return {"A": int(A), "hq": rows[0], "lq": rows[1], "n": rows[2] if separate_n else None, "lq_map": lq_map, "n_map": n_map}


def state_with_counts(rng, L, separate_n, counts):
    """a valid state with exactly counts = (HQ, LQ, N) reads (N ignored without an N set), the classes in random order"""
    nh, nl, nn = counts[0], counts[1], counts[2] if separate_n else 0
    sym, rb = set_shapes(L, separate_n)
    cls = rng.permutation(np.repeat(np.arange(3, dtype=np.uint8), [nh, nl, nn]))
    A = int(cls.size)
    rows = [rng.integers(0, 125 if sym[k] == 5 else 256, size=(c, rb[k]), dtype=np.uint8) for k, c in enumerate((nh, nl, nn))]
    lq_map = np.concatenate([np.flatnonzero(cls == 1), [A]]).astype(np.uint32)
    n_map = np.concatenate([np.flatnonzero(cls == 2), [A]]).astype(np.uint32) if separate_n else None
    return {"A": A, "hq": rows[0], "lq": rows[1], "n": rows[2] if separate_n else None, "lq_map": lq_map, "n_map": n_map}


def state_batch(st, L, separate_n, n_reads_lq=False):
    """the state as ONE batch of the divider (DividedPCLReadsSets.divide's dict)"""
    sym, rb = set_shapes(L, separate_n, n_reads_lq)
    n_rows = st["n"] if st["n"] is not None else np.zeros((0, 0), np.uint8)
    n_idx = st["n_map"][:-1] if st["n_map"] is not None else np.zeros(0, np.uint32)
    return {"n_hq": st["hq"].shape[0], "n_lq": st["lq"].shape[0], "n_n": n_rows.shape[0], "symbols": sym, "row_bytes": rb,
            "hq_rows": st["hq"], "lq_rows": st["lq"], "n_rows": n_rows, "lq_index": st["lq_map"][:-1], "n_index": n_idx}


def split_batches(st, L, separate_n, cuts):
    """the state as the batches of the records [cuts[i], cuts[i + 1]): (batch, n_records) each, the indexes batch-local"""
    sym, rb = set_shapes(L, separate_n)
    A = st["A"]
    cls = np.zeros(A, np.uint8)
    cls[st["lq_map"][:-1]] = 1
    if st["n_map"] is not None:
        cls[st["n_map"][:-1]] = 2
    rows = [st["hq"], st["lq"], st["n"] if st["n"] is not None else np.zeros((0, 0), np.uint8)]
    at = [0, 0, 0]
    out = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        c = cls[lo:hi]
        cnt = [int((c == k).sum()) for k in range(3)]
        part = [rows[k][at[k]:at[k] + cnt[k]] for k in range(3)]
        for k in range(3):
            at[k] += cnt[k]
        out.append(({"n_hq": cnt[0], "n_lq": cnt[1], "n_n": cnt[2], "symbols": sym, "row_bytes": rb, "hq_rows": part[0],
                     "lq_rows": part[1], "n_rows": part[2], "lq_index": np.flatnonzero(c == 1).astype(np.uint32),
                     "n_index": np.flatnonzero(c == 2).astype(np.uint32)}, hi - lo))
    return out


# ------------------------------------------------------------------------------------------------ the reference's loops
def literal_move(st, is_hq):
    """moveLqReadsFromHqReadsSetsToLqReadsSets, :145-197"""
    st = copy_state(st)
    hq, lq = st["hq"], st["lq"]
    separate_n = st["n_map"] is not None
    to_move = int(sum(1 for f in is_hq if not f))
    new_lq = lq.shape[0] + to_move
    lq_counter = lq.shape[0]
    ignore_lq = lq_counter == 0
    lq_counter = (lq_counter - 1) & M32
    # (a row is copied as its number in `src`, and the rows are gathered at the end: the loops are the reference's, a copyRead is an int)
    src = np.concatenate([lq, hq]) if lq.shape[1] == hq.shape[1] else lq
    n_lq_old = lq.shape[0]
    lq = list(range(n_lq_old)) + [-1] * to_move                                           # lqReadsSet->resize(newLqCounter)
    idx = [int(x) for x in st["lq_map"]]
    idx = idx[:new_lq + 1] + [0] * (new_lq + 1 - len(idx))                                # lqReadIdx.resize(newLqCounter + 1)
    all_counter = st["A"]
    idx[new_lq] = all_counter
    new_lq_counter = (new_lq - 1) & M32
    n_counter = st["n"].shape[0] if separate_n else 0
    n_map = [int(x) for x in st["n_map"]] if separate_n else []
    is_hq = [bool(x) for x in is_hq]
    ignore_n = n_counter == 0
    n_counter = (n_counter - 1) & M32
    hq_counter = hq.shape[0]
    while True:
        go = all_counter > 0
        all_counter = (all_counter - 1) & M32
        if not (go and hq_counter != 0):
            break
        if not ignore_n:
            if n_map[n_counter] == all_counter:
                ignore_n = n_counter == 0
                n_counter = (n_counter - 1) & M32
                continue
        if not ignore_lq:
            if idx[lq_counter] == all_counter:
                lq[new_lq_counter] = lq[lq_counter]
                idx[new_lq_counter] = all_counter
                ignore_lq = lq_counter == 0
                lq_counter = (lq_counter - 1) & M32
                last = new_lq_counter == 0
                new_lq_counter = (new_lq_counter - 1) & M32
                if last:
                    break
                continue
        hq_counter -= 1
        if not is_hq[hq_counter]:
            lq[new_lq_counter] = n_lq_old + hq_counter
            idx[new_lq_counter] = all_counter
            last = new_lq_counter == 0
            new_lq_counter = (new_lq_counter - 1) & M32
            if last:
                break
    new_hq = 0
    hq_tok = list(range(hq.shape[0]))
    for h in range(hq.shape[0]):
        if is_hq[h]:
            hq_tok[new_hq] = hq_tok[h]
            new_hq += 1
    st["hq"] = hq[np.array(hq_tok[:hq.shape[0] - to_move], dtype=np.int64)]
    assert -1 not in lq
    st["lq"] = src[np.array(lq, dtype=np.int64)] if lq else st["lq"][:0]
    st["lq_map"] = np.array(idx, dtype=np.uint32)
    return st


def literal_hq_mapping(st):
    """generateHqReadsIndexesMapping, :199-216"""
    out = []
    lq_counter = n_counter = 0
    lq_map = [int(x) for x in st["lq_map"]]
    n_map = [int(x) for x in st["n_map"]] if st["n_map"] is not None else None
    for a in range(st["A"]):
        if lq_map[lq_counter] == a:
            lq_counter += 1
        elif n_map is not None and n_map[n_counter] == a:
            n_counter += 1
        else:
            out.append(a)
    return np.array(out + [st["A"]], dtype=np.uint32)


def _literal_remove_one(rows, mapping, flags, beg, A):
    tok = list(range(rows.shape[0]))
    idx = [int(x) for x in mapping]
    flags = [bool(x) for x in flags]
    new = 0
    for i in range(rows.shape[0]):
        if not flags[i + beg]:
            idx[new] = idx[i]
            tok[new] = tok[i]
            new += 1
    idx[new] = A
    return rows[np.array(tok[:new], dtype=np.int64)], np.array(idx[:new + 1], dtype=np.uint32)


def literal_remove(st, is_mapped):
    """removeReadsFromLqReadsSet(flags), then removeReadsFromNReadsSet(flags, nBegIdx = the LQ count before), as
    pgrc-encoder.cpp:367-372 calls them"""
    st = copy_state(st)
    n_beg = st["lq"].shape[0]
    st["lq"], st["lq_map"] = _literal_remove_one(st["lq"], st["lq_map"], is_mapped, 0, st["A"])
    if st["n_map"] is not None:
        st["n"], st["n_map"] = _literal_remove_one(st["n"], st["n_map"], is_mapped, n_beg, st["A"])
    return st


# ------------------------------------------------------------------------------------------------ the class-space form
def classes(st):
    cls = np.zeros(st["A"], np.uint8)
    cls[st["lq_map"][:-1]] = 1
    if st["n_map"] is not None:
        cls[st["n_map"][:-1]] = 2
    return cls


def class_move(st, is_hq):
    st = copy_state(st)
    A = st["A"]
    is_hq = np.asarray(is_hq, dtype=bool)
    cls = classes(st)
    hq_rank = np.cumsum(cls == 0) - (cls == 0)                   # exclusive counts: the old HQ rows in front of an index
    lq_rank = np.cumsum(cls == 1) - (cls == 1)
    hq_idx = np.flatnonzero(cls == 0)
    cls[hq_idx[~is_hq]] = 3
    to_lq = np.flatnonzero((cls == 1) | (cls == 3))
    src = np.concatenate([st["lq"], st["hq"]])                   # the descriptor's top bit: the second array
    desc = np.where(cls[to_lq] == 1, lq_rank[to_lq], st["lq"].shape[0] + hq_rank[to_lq])
    st["lq"] = src[desc] if desc.size else st["lq"][:0]
    st["lq_map"] = np.concatenate([to_lq, [A]]).astype(np.uint32)
    st["hq"] = st["hq"][hq_rank[np.flatnonzero(cls == 0)]]
    return st


def class_hq_mapping(st):
    return np.concatenate([np.flatnonzero(classes(st) == 0), [st["A"]]]).astype(np.uint32)


def class_remove(st, is_mapped):
    st = copy_state(st)
    f = np.asarray(is_mapped, dtype=bool)
    nl = st["lq"].shape[0]
    keep = ~f[:nl]
    st["lq"] = st["lq"][keep]
    st["lq_map"] = np.concatenate([st["lq_map"][:-1][keep], [st["A"]]]).astype(np.uint32)
    if st["n_map"] is not None:
        keep = ~f[nl:nl + st["n"].shape[0]]
        st["n"] = st["n"][keep]
        st["n_map"] = np.concatenate([st["n_map"][:-1][keep], [st["A"]]]).astype(np.uint32)
    return st


def same_state(a, b):
    for k in ("hq", "lq", "n", "lq_map", "n_map"):
        if (a[k] is None) != (b[k] is None):
            return False
        if a[k] is not None and (a[k].shape[0] != b[k].shape[0] or not np.array_equal(a[k], b[k])):
            return False
    return a["A"] == b["A"]


def device_state(sets):
    """the state held by a pgrc_amd.DividedReadsSets"""
    i = sets.info()
    have_n = i["symbols"][2] != 0
    return {"A": i["reads_total_count"], "hq": sets.get_rows("hq"), "lq": sets.get_rows("lq"), "n": sets.get_rows("n") if have_n else None,
            "lq_map": sets.get_mapping("lq"), "n_map": sets.get_mapping("n") if have_n else None}


def load_fixture(name):
    """a fixture of tests/golden/make_golden_rsets.py: (L, separate_n, before, is_hq, after_move, hq_mapping, is_mapped, after_remove)"""
    z = np.load(os.path.join(GOLDEN, name))
    sep = bool(z["separate_n"])

    def state(p):
        return {"A": int(z["A"]), "hq": z[p + "hq"], "lq": z[p + "lq"], "n": z[p + "n"] if sep else None, "lq_map": z[p + "lq_map"],
                "n_map": z[p + "n_map"] if sep else None}
    return {"L": int(z["L"]), "separate_n": sep, "before": state("b_"), "is_hq": z["is_hq"], "moved": state("m_"), "hq_mapping": z["hq_mapping"],
            "is_mapped": z["is_mapped"], "removed": state("r_")}
