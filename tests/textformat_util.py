"""FASTA and one-read-per-line sources (test infrastructure): a plain restatement of the reference's two iterators
(FASTAReadsSourceIterator and ConcatenatedReadsSourceIterator, readsset/iterator/ReadsSetIterator.cpp:118-134 and :66-76) and of
the pairing and the reverse complement around them (ManagedReadsSetIterator, RevComplPairReadsSetIterator), record by record;
writers of such files with everything a line can carry; and the piece-wise feeding of pgrc_divider_run_text."""
import numpy as np

FASTQ, FASTA, LINES = 0, 1, 2
E_PARAM, E_SYMBOL = 1, 5
# PgHelpers' complement table (utils/helper.cpp:261-282): both cases map to the upper-case complement, everything else to 0
_COMPLEMENT = {}
for _a, _b in ("AT", "CG", "GC", "TA", "NN", "UA", "YR", "RY", "KM", "MK", "BV", "DH", "HD", "VB"):
    _COMPLEMENT[ord(_a)] = _COMPLEMENT[ord(_a.lower())] = ord(_b)


def getlines(text):
    """std::getline until it fails: a last line without a newline counts, nothing follows a last newline"""
    lines = bytes(text).split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def read_lines(fmt, text):
    """the lines the iterator stops at: every line (LINES), every line whose first byte is neither '>' nor ';' (FASTA)"""
    lines = getlines(text)
    return lines if fmt == LINES else [ln for ln in lines if ln[:1] not in (b">", b";")]


def leading_letters(line):
    k = 0
    while k < len(line) and (65 <= line[k] <= 90 or 97 <= line[k] <= 122):     # isalpha in the C locale
        k += 1
    return line[:k]


def restate(fmt, text, pair_text, rev_compl_pair, L):
    """-> the (n, L) rows in record order, or E_PARAM / E_SYMBOL: what the first record the reference cannot take makes it.
    LINES never looks at a pair file (the reference hands it no second stream)."""
    src = [read_lines(fmt, text)]
    if pair_text is not None and fmt == FASTA:
        src.append(read_lines(fmt, pair_text))
    at, rows, k = [0] * len(src), [], 0
    while True:
        f = k % len(src)
        if at[f] == len(src[f]):
            break                                            # the source whose turn it is has no more: the iteration ends
        read = leading_letters(src[f][at[f]])
        at[f] += 1
        if len(read) != L:
            return E_PARAM                                   # "Unsupported variable length reads"
        if f == 1 and rev_compl_pair:
            read = bytes(_COMPLEMENT.get(c, 0) for c in reversed(read))
        if any(c not in b"ACGNT" for c in read):
            return E_SYMBOL
        rows.append(np.frombuffer(read, np.uint8))
        k += 1
    return np.stack(rows) if rows else np.zeros((0, L), np.uint8)


def write_fasta(reads, seed=0, crlf=False, trailing_newline=True, comments=False, multi_headers=False, header_last=False,
                tail_text=False):
    """one read per record behind a '>' line of varying length.  comments: ';' lines in front of some records (the first line
    of the file included, every 11th record); multi_headers: two or three header lines in a row here and there; header_last:
    the file ends with a header line (which, with trailing_newline off, is the line without a newline); tail_text: blanks
    and more text behind the read on its line"""
    rng = np.random.default_rng(seed)
    nl = b"\r\n" if crlf else b"\n"
    parts = []
    for i in range(reads.shape[0]):
        if comments and i % 11 == 0:
            parts += [b";comment %d" % i + b"y" * int(rng.integers(0, 9)), nl]
        parts += [b">r%d" % i + b"x" * int(rng.integers(0, 40)), nl]
        if multi_headers and i % 7 == 3:
            parts += [b">again", nl] * (1 + i % 2) + [b";", nl]
        parts += [reads[i].tobytes(), (b" len=%d\tACGT" % reads.shape[1]) if tail_text and i % 3 == 1 else b"", nl]
    if header_last:
        parts += [b">the end", nl]
    text = b"".join(parts)
    return text if trailing_newline or not parts else text[: -len(nl)]


def write_lines(reads, crlf=False, trailing_newline=True, tail_text=False):
    nl = b"\r\n" if crlf else b"\n"
    parts = []
    for i in range(reads.shape[0]):
        parts += [reads[i].tobytes(), b" 7" if tail_text and i % 3 == 1 else b"", nl]
    text = b"".join(parts)
    return text if trailing_newline or not parts else text[: -len(nl)]


def concat(parts):
    """division results of consecutive pieces -> (one result, records): indexes shifted by the records before"""
    out = {k: parts[0][0][k] for k in ("symbols", "row_bytes")}
    acc = {k: [] for k in ("hq_rows", "lq_rows", "n_rows", "lq_index", "n_index")}
    tot, base = {"n_hq": 0, "n_lq": 0, "n_n": 0}, 0
    for res, nrec in parts:
        for k in ("hq_rows", "lq_rows", "n_rows"):
            acc[k].append(res[k])
        acc["lq_index"].append(res["lq_index"] + np.uint32(base))
        acc["n_index"].append(res["n_index"] + np.uint32(base))
        for k in tot:
            tot[k] += res[k]
        base += nrec
    out.update(tot)
    out.update({k: np.concatenate(v) for k, v in acc.items()})
    return out, base


def feed(d, fmt, text, pair_text, rev, cuts, pair_cuts=None):
    """the texts through d.divide_text in pieces that end at the given offsets (ascending, the last one the text's length),
    what a call leaves unconsumed handed over again in front of the next piece; the call at which both texts are through is
    the final one.  -> (result, records, terminal flag of the last call, calls)"""
    src = [text] + ([] if pair_text is None else [pair_text])
    cuts = [list(cuts)] + ([] if pair_text is None else [list(pair_cuts if pair_cuts is not None else cuts)])
    for f in range(len(src)):                                # both lists as long as the longer one: a text that is through stays
        cuts[f] = [min(c, len(src[f])) for c in cuts[f]]
    steps = max(len(c) for c in cuts)
    at, parts = [0] * len(src), []
    for k in range(steps):
        have = [c[min(k, len(c) - 1)] for c in cuts]
        final = k == steps - 1
        assert not final or all(h == len(s) for h, s in zip(have, src))
        res, nrec, used, pused = d.divide_text(fmt, src[0][at[0]: have[0]], src[1][at[1]: have[1]] if len(src) > 1 else None, rev, final=final)
        assert used <= have[0] - at[0] and (len(src) == 1 or pused <= have[1] - at[1])
        parts.append((res, nrec))
        at[0] += used
        if len(src) > 1:
            at[1] += pused
    res, n = concat(parts)
    return res, n, d.last_was_terminal(), steps


def piece_cuts(length, piece):
    return list(range(piece, length, piece)) + [length]
