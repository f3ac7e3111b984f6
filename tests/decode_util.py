"""numpy restatement of the reference decoder's read rebuild (the checker of include/pgrc_decode.h), and the decode cases
of the tests: a separated-pseudogenome job (HQ text + its reads list from the export streams, LQ and N texts made of the
unmatched reads) with its ground truth, which is the input reads themselves.

Restated (pgrc/ and pseudogenome/ of the reference):
  per entry     SeparatedPseudoGenome::getRead* (SeparatedPseudoGenome.cpp:74-120): window text[pos, pos+L), reversed and
                complemented in place when revComp (complementsLut, utils/helper.cpp:243-262), then for every mismatch i
                ptr[misOff[i]] = code2mismatch(ptr[misOff[i]], misSymCode[i]) (helper.cpp:353-356) under the order of
                reorderSymAndVal(basesOrder)
  positions     inclusive scan of the offset deltas (enableConstantAccess, SeparatedExtendedReadsList.cpp:328-363)
  offsets       convertMisRevOffsets2Offsets (utils/helper.h:52-63)
  writers       writeAllReadsInSEMode* :137-239, PEMode* :241-383, ORDMode* :385-527 (pgrc/pgrc-decoder.cpp); entries are
                numbered HQ, LQ, N (rlIdx); LQ and N rows carry no RC flags and no mismatches and are reverse-complemented
                in file 2; applyRevComplPairFileToPgs (:700-724) flips the HQ RC flag of file 2's rows
  symbol order  SeparatedPseudoGenomeOutputBuilder::reorderingSymbolsExclusiveMismatchEncoding
                (SeparatedPseudoGenomePersistence.cpp:1115-1138)
"""
import numpy as np

ACGTN = b"ACGTN"

COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in ("AT", "CG", "GC", "TA", "NN", "UA", "YR", "RY", "KM", "MK", "BV", "DH", "HD", "VB"):
    COMP[ord(_a)] = COMP[ord(_a.lower())] = ord(_b)


def revcomp_rows(rows):
    return COMP[rows[:, ::-1]]


def with_newlines(rows):
    out = np.empty((rows.shape[0], rows.shape[1] + 1), dtype=np.uint8)
    out[:, :-1] = rows
    out[:, -1] = ord("\n")
    return out


# ---------------------------------------------------------------- mismatch streams
def rev_offsets_to_offsets(mis_cnt, mis_rev_off, L):
    """convertMisRevOffsets2Offsets per entry: the stream holds r_{m-1} .. r_0; walking it, pos -= r + 1 gives
    off_{m-1} .. off_0 (returned in list order off_0 .. off_{m-1})"""
    cnt = np.asarray(mis_cnt, dtype=np.int64)
    r = np.asarray(mis_rev_off, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    eid = np.repeat(np.arange(cnt.size), cnt)
    k = np.arange(r.size) - starts[eid]
    cs = np.cumsum(r + 1)
    cs_before = np.concatenate([[0], cs])[starts[eid]]
    fwd = L - (cs - cs_before)
    out = np.empty(r.size, dtype=np.int64)
    out[starts[eid] + cnt[eid] - 1 - k] = fwd
    assert (out >= 0).all() and (out < L).all()
    return out


def offsets_to_rev_offsets(mis_cnt, offsets, L):
    """the inverse (writeReadEntry, SeparatedPseudoGenomePersistence.cpp:975-981)"""
    cnt = np.asarray(mis_cnt, dtype=np.int64)
    off = np.asarray(offsets, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    out = np.empty(off.size, dtype=np.int64)
    for e in np.flatnonzero(cnt):
        s, m = starts[e], cnt[e]
        cur = L - 1
        for j, i in enumerate(range(m - 1, -1, -1)):
            out[s + j] = cur - off[s + i]
            cur = off[s + i] - 1
    return out


def exclusive_encoding(mis_sym_ctx):
    """reorderingSymbolsExclusiveMismatchEncoding: symbols ordered by descending count of mismatch values (std::sort of
    five values: an insertion sort, so ties keep the order A C G T N), codes made exclusive of the actual value ->
    (codes, bases order)"""
    c = np.asarray(mis_sym_ctx, dtype=np.uint8)
    counts = np.bincount(c & 15, minlength=5)[:5]
    order = sorted(range(5), key=lambda v: -counts[v])
    rev = np.zeros(16, dtype=np.int64)
    rev[order] = np.arange(5)
    av, mv = rev[c >> 4], rev[c & 15]
    codes = (mv - (mv > av)).astype(np.uint8)
    return codes, bytes(ACGTN[v] for v in order)


def code2mismatch(actual, code, order):
    s2v = np.full(256, 255, dtype=np.int64)
    s2v[np.frombuffer(order, dtype=np.uint8)] = np.arange(5)
    av = s2v[actual]
    code = code.astype(np.int64)
    return np.frombuffer(order, dtype=np.uint8)[np.where(code < av, code, code + 1)]


# ---------------------------------------------------------------- the per-entry rule and the writers
def hq_rows(text, L, pos, rc, lst, entries):
    """rows of HQ entries `entries` with windows at joined positions `pos` and RC flags `rc` (already flipped where the
    pair-file rule says so), their mismatches applied in list order"""
    rows = text[np.asarray(pos, dtype=np.int64)[:, None] + np.arange(L)]
    rc = np.asarray(rc, dtype=bool)
    rows[rc] = revcomp_rows(rows[rc])
    if lst.get("mis_cnt") is None or not len(entries):
        return rows
    cnt = np.asarray(lst["mis_cnt"], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(cnt)])
    off = lst["mis_off"]
    off = rev_offsets_to_offsets(cnt, off, L) if lst["rev_coded"] else np.asarray(off, dtype=np.int64)
    sym = np.asarray(lst["mis_sym"], dtype=np.uint8)
    e = np.asarray(entries, dtype=np.int64)
    m = cnt[e]
    for k in range(int(m.max()) if m.size else 0):       # mismatch k of every entry that has one, in list order
        r = np.flatnonzero(m > k)
        i = starts[e[r]] + k
        o = off[i]
        if lst["form"] == 1:
            rows[r, o] = np.frombuffer(ACGTN, dtype=np.uint8)[sym[i] & 15]
        else:
            rows[r, o] = code2mismatch(rows[r, o], sym[i], lst.get("order") or ACGTN)
    return rows


def list_positions(lst):
    if lst.get("pos") is not None:
        return lst["text_base"] + np.asarray(lst["pos"], dtype=np.int64)
    return lst["text_base"] + np.cumsum(np.asarray(lst["off"], dtype=np.int64))


def write_se(dc):
    """writeAllReadsInSEMode*: every list in list order"""
    L, text, lists = dc["L"], dc["text"], dc["lists"]
    hq = lists[0]
    n0 = hq["n"]
    rc0 = np.zeros(n0, bool) if hq.get("rc") is None else hq["rc"].astype(bool)
    parts = [hq_rows(text, L, list_positions(hq), rc0, hq, np.arange(n0))]
    for lst in lists[1:]:
        parts.append(text[list_positions(lst)[:, None] + np.arange(L)])
    return with_newlines(np.concatenate(parts) if parts else np.zeros((0, L), np.uint8))


def write_pe(dc, rl_idx_order, pair_file):
    """writeAllReadsInPEMode*: file p = rows i = p (mod 2) of rlIdxOrder -> (file 1, file 2)"""
    L, text, lists = dc["L"], dc["text"], dc["lists"]
    hq = lists[0]
    n0 = hq["n"]
    pos_all = np.concatenate([list_positions(x) for x in lists])
    rc0 = np.zeros(n0, bool) if hq.get("rc") is None else hq["rc"].astype(bool)
    out = []
    for p in range(2):
        idx = np.asarray(rl_idx_order, dtype=np.int64)[p::2]
        rows = np.empty((idx.size, L), dtype=np.uint8)
        h = idx < n0
        rows[h] = hq_rows(text, L, pos_all[idx[h]], rc0[idx[h]] ^ bool(pair_file and p == 1), hq, idx[h])
        raw = text[pos_all[idx[~h]][:, None] + np.arange(L)]
        rows[~h] = revcomp_rows(raw) if p == 1 else raw
        out.append(with_newlines(rows))
    return tuple(out)


def write_ord(dc, org2pos, paired, pair_file):
    """writeAllReadsInORDMode*: row i of file p = orgIdx2PgPos[(T / parts) * p + i]; rows below hqPgLen take the HQ entries
    (their RC flags and mismatches) in the order they appear"""
    L, text, lists = dc["L"], dc["text"], dc["lists"]
    hq = lists[0]
    hq_len = lists[1]["text_base"] if len(lists) > 1 else text.size
    org2pos = np.asarray(org2pos, dtype=np.int64)
    T = org2pos.size
    is_hq = org2pos < hq_len
    rank = np.cumsum(is_hq) - is_hq
    rc0 = np.zeros(hq["n"], bool) if hq.get("rc") is None else hq["rc"].astype(bool)
    parts = 2 if paired else 1
    out = []
    for p in range(parts):
        i = np.arange((T // parts) * p, (T // parts) * (p + 1))
        rows = np.empty((i.size, L), dtype=np.uint8)
        h = is_hq[i]
        flip = bool(pair_file) & (i[h] >= T // 2)
        rows[h] = hq_rows(text, L, org2pos[i[h]], rc0[rank[i[h]]] ^ flip, hq, rank[i[h]])
        raw = text[org2pos[i[~h]][:, None] + np.arange(L)]
        rows[~h] = revcomp_rows(raw) if p == 1 else raw
        out.append(with_newlines(rows))
    return tuple(out)


# ---------------------------------------------------------------- decode cases built from the export streams
def close_list(case, seed=0, even=False):
    """the old reads list of an export case extended to the end of the Pg, as every HQ list of PgRC is (its last read
    ends where the text ends): entries at most 255 apart up to position G - L, with new original indexes.  An export
    whose matches lie beyond the old list's last entry writes their offsets from -1 (writeReadsFromIterator returns -1
    once the list is exhausted, SeparatedPseudoGenomePersistence.cpp:1018): such an archive does not decode to its
    reads, in the reference as here.  even: the total made even (a paired job's; ORD's two halves need it)."""
    c = dict(case)
    off = np.asarray(case["list_off"], np.int64)
    end = len(case["pg"]) - case["L"]
    cur = int(off.sum()) if off.size else 0
    add = []
    while cur < end:
        step = min(200, end - cur) if (off.size or add) else min(200, end)
        add.append(step)
        cur += step
    if even and (case["total"] + len(add)) % 2:
        add.append(0)                # a paired job has an even number of reads: one more entry at the last position
    rng = np.random.default_rng(seed)
    k = len(add)
    c["list_off"] = np.concatenate([off, add]).astype(np.uint8)
    c["list_org"] = np.concatenate([case["list_org"], case["total"] + np.arange(k)]).astype(np.uint32)
    c["list_rc"] = np.concatenate([case["list_rc"], rng.random(k) < 0.4]).astype(np.uint8)
    c["total"] = case["total"] + k
    return c


def sane_hq_entries(case, res, pg_st):
    """the Pg-order entries whose offsets give their true position: all of them, unless matches lie beyond the old
    list's last entry (see close_list)"""
    pos = np.cumsum(pg_st["off"].astype(np.int64))
    owner = np.full(case["total"], -1, np.int64)
    owner[np.asarray(case["read_org"], np.int64)] = np.arange(len(case["read_org"]))
    org = pg_st["org_idx"].astype(np.int64)
    lpos = np.cumsum(np.asarray(case["list_off"], np.int64))
    lidx = np.full(case["total"], -1, np.int64)
    lidx[np.asarray(case["list_org"], np.int64)] = np.arange(lpos.size)
    r = owner[org]
    true = np.where(r >= 0, np.asarray(res["pos"], np.int64)[np.maximum(r, 0)], lpos[np.maximum(lidx[org], 0)])
    return pos == true


def streams_from_bytes(b):
    """stream files' bytes (byte-per-read-length mode) -> arrays"""
    return {"off": np.frombuffer(b["off"], np.uint8), "org_idx": np.frombuffer(b["org_idx"], np.uint32),
            "rev_comp": np.frombuffer(b["rev_comp"], np.uint8), "mis_cnt": np.frombuffer(b["mis_cnt"], np.uint8),
            "mis_sym": np.frombuffer(b["mis_sym"], np.uint8), "mis_rev_off": np.frombuffer(b["mis_rev_off"], np.uint8)}


def hq_list(st, L, with_pos=True, wide=False, archive=False):
    """the HQ list of a decode case from export streams: context codes as exported (form 1) or the archive's exclusive
    codes (form 0, reordered symbols); one- or two-byte offsets"""
    w = np.uint16 if wide else np.uint8
    lst = {"text_base": 0, "n": st["org_idx"].size, "rc": st["rev_comp"].copy(), "mis_cnt": st["mis_cnt"].copy(),
           "mis_off": st["mis_rev_off"].astype(w), "rev_coded": True, "form": 1, "mis_sym": st["mis_sym"].copy()}
    if with_pos:
        lst["off"] = st["off"].astype(w)
    if archive:
        lst["mis_sym"], lst["order"] = exclusive_encoding(st["mis_sym"])
        lst["form"] = 0
    return lst


def decode_case(case, res, pg_st, org_st=None, pair=False, wide=False, archive=False):
    """-> dict: joined text, L, the lists of SE / PE order (HQ from the Pg-order streams), the ORD lists (HQ from the
    original-order streams), rlIdxOrder, orgIdx2PgPos, and the ground truth of every original index (its read, or
    the Pg window of an old list entry / a filler) with the kind of list it sits in"""
    L, pg, reads = case["L"], np.asarray(case["pg"], np.uint8), np.asarray(case["reads"], np.uint8)
    n, n_n, T = reads.shape[0], case["n_n"], case["total"]
    read_org = np.asarray(case["read_org"], np.int64)
    um = np.asarray(res["mism"]) == 255
    lq = np.flatnonzero(um[: n - n_n])
    nn = (n - n_n) + np.flatnonzero(um[n - n_n:])
    hq_len, lq_len = pg.size, lq.size * L
    text = np.concatenate([pg, reads[lq].reshape(-1), reads[nn].reshape(-1)]).astype(np.uint8)
    step = np.full(max(lq.size, nn.size), L, dtype=np.uint16 if wide else np.uint8)
    lq_list = {"text_base": hq_len, "n": lq.size, "off": np.concatenate([[0], step[: max(lq.size - 1, 0)]])[: lq.size].astype(step.dtype)}
    n_list = {"text_base": hq_len + lq_len, "n": nn.size, "off": np.concatenate([[0], step[: max(nn.size - 1, 0)]])[: nn.size].astype(step.dtype)}
    hq = hq_list(pg_st, L, wide=wide, archive=archive)
    # ground truth by original index
    truth = np.zeros((T, L), dtype=np.uint8)
    kind = np.zeros(T, dtype=np.int8)            # 0 HQ, 1 LQ, 2 N
    matched = np.flatnonzero(~um)
    truth[read_org[matched]] = reads[matched]
    lpos = np.cumsum(np.asarray(case["list_off"], np.int64))
    lw = pg[lpos[:, None] + np.arange(L)] if lpos.size else np.zeros((0, L), np.uint8)
    lrc = np.zeros(lpos.size, bool) if case["list_rc"] is None else np.asarray(case["list_rc"], bool)
    lw[lrc] = revcomp_rows(lw[lrc])
    truth[np.asarray(case["list_org"], np.int64)] = lw
    truth[read_org[lq]] = reads[lq]
    kind[read_org[lq]] = 1
    truth[read_org[nn]] = reads[nn]
    kind[read_org[nn]] = 2
    # rlIdx of every original index
    rl_of_org = np.full(T, -1, dtype=np.int64)
    rl_of_org[pg_st["org_idx"]] = np.arange(pg_st["org_idx"].size)
    rl_of_org[read_org[lq]] = hq["n"] + np.arange(lq.size)
    rl_of_org[read_org[nn]] = hq["n"] + lq.size + np.arange(nn.size)
    assert (rl_of_org >= 0).all()
    dc = {"L": L, "text": text, "lists": [hq, lq_list, n_list], "rl_idx_order": rl_of_org.astype(np.uint32),
          "truth": truth, "kind": kind, "pair": pair, "T": T}
    if org_st is not None:
        # ORD: the HQ list of the original-order export (no positions needed), orgIdx2PgPos in row order
        dc["ord_lists"] = [hq_list(org_st, L, with_pos=False, wide=wide, archive=archive), lq_list, n_list]
        hq_pos = np.zeros(T, dtype=np.int64)           # fillers: position 0
        owner = np.full(T, -1, dtype=np.int64)
        owner[read_org] = np.arange(n)
        o = org_st["org_idx"].astype(np.int64)
        r = owner[o]
        hq_pos[o[r >= 0]] = np.asarray(res["pos"], np.int64)[r[r >= 0]]
        pos_of_org = hq_pos
        pos_of_org[read_org[lq]] = hq_len + np.arange(lq.size) * L
        pos_of_org[read_org[nn]] = hq_len + lq_len + np.arange(nn.size) * L
        dc["ord_org_of_row"] = ord_org_of_row(T, pair)
        dc["org2pos"] = pos_of_org[dc["ord_org_of_row"]].astype(np.uint64)
        dc["filler"] = np.zeros(T, bool)
        dc["filler"][np.asarray(case["list_org"], np.int64)] = True
    return dc


def ord_org_of_row(T, paired):
    """the original index of ORD row i (preparePgsForValidation, pgrc-decoder.cpp:557-559): parts of T/parts rows"""
    i = np.arange(T)
    if not paired:
        return i
    h = T // 2
    return np.where(i < h, 2 * i, np.where(i < 2 * h, 2 * (i - h) + 1, T - 1))     # (an odd T's last row is never written)


def truth_rows_pe(dc, p):
    """ground truth of PE file p: the read (or Pg window) of original index 2r + p; in file 2 the LQ / N rows are
    reverse-complemented, and the HQ rows too when the pair-file rule is on"""
    o = np.arange(p, dc["T"], 2)
    rows = dc["truth"][o].copy()
    if p == 1:
        rc = (dc["kind"][o] > 0) | bool(dc["pair"])
        rows[rc] = revcomp_rows(rows[rc])
    return with_newlines(rows)


def truth_rows_ord(dc, text, p, paired):
    """ground truth of ORD file p: the read of the row's original index; fillers (old list entries, exported without a
    read) are the window at position 0; orientation as in PE"""
    T = dc["T"]
    parts = 2 if paired else 1
    i = np.arange((T // parts) * p, (T // parts) * (p + 1))
    o = dc["ord_org_of_row"][i]
    rows = dc["truth"][o].copy()
    f = dc["filler"][o]
    rows[f] = text[np.arange(dc["L"])][None, :]
    if p == 1:
        rc = (dc["kind"][o] > 0) | bool(dc["pair"])
        rows[rc] = revcomp_rows(rows[rc])
    return with_newlines(rows)


def truth_rows_se(dc, pg_st, case, res):
    """ground truth of SE: HQ entries in list order (by their original index), then the LQ and N reads"""
    L = dc["L"]
    rows = [dc["truth"][pg_st["org_idx"].astype(np.int64)]]
    text = dc["text"]
    for lst in dc["lists"][1:]:
        rows.append(text[list_positions(lst)[:, None] + np.arange(L)])
    return with_newlines(np.concatenate(rows))
