"""FASTA and one-read-per-line text parsed on the device (pgrc_divider_run_text, pgrc_verify_add_text): against
tests/textformat_util.py's restatement of the reference's iterators everywhere, and against the compiled reference's own managed
iterator where oracle/_ref is present.  Whole files and pieces cut at every kind of place; the refusals, each followed by a good
file on the same divider; FASTQ forwarding; the hand-over to the resident read sets; the verifier."""
import numpy as np
import pytest

import oracle as orc
import rsets_util as ru
import textformat_util as tu
from divide_util import COMBOS, make_fastq, make_records, oracle_divide, oracle_divide_fastq, ref_divide_files, same
from pgrc_amd import DividedPCLReadsSets, DividedReadsSets, PgrcMatchError, Verifier

pytestmark = pytest.mark.gpu

HAVE_REF = orc.have_ref() and hasattr(orc.ref(), "pgrc_ref_divide_files")
SEP_N, N_LQ = COMBOS[1], COMBOS[2]                  # separate_n and n_reads_lq, both with error_limit 1
SIZES = [(21, 300), (100, 1200)]
PIECES = (64, 257, 5000)

_records = {}


def records(L, n):
    if (L, n) not in _records:
        _records[(L, n)] = make_records(seed=3 * L + n, n=n, L=L, n_frac=0.1)[0]
        _records[(L, n)].setflags(write=False)
    return _records[(L, n)]


def expected(fmt, a, b, rev, L, combo, tmp_path=None):
    """the restatement's rows through the oracle division; with oracle/_ref the reference's own result must be the same"""
    rows = tu.restate(fmt, a, b, rev, L)
    assert isinstance(rows, np.ndarray)
    want = oracle_divide(rows, None, *combo) if rows.shape[0] else None
    if HAVE_REF and tmp_path is not None and rows.shape[0]:
        (tmp_path / "a.txt").write_bytes(a)
        if b is not None:
            (tmp_path / "b.txt").write_bytes(b)
        ref = ref_divide_files(tmp_path / "a.txt", tmp_path / "b.txt" if b is not None else None, rev, L, rows.shape[0] + 8, combo)
        assert same(want, ref) is None, same(want, ref)
    return want, rows.shape[0]


def whole(fmt, a, b, rev, L, combo):
    d = DividedPCLReadsSets(L, *combo)
    res, nrec, used, pused = d.divide_text(fmt, a, b, rev, final=True)
    terminal = d.last_was_terminal()
    d.close()
    return res, nrec, used, pused, terminal


def check_whole_and_pieces(fmt, a, b, rev, L, combo, tmp_path, extra_cuts=()):
    want, n = expected(fmt, a, b, rev, L, combo, tmp_path)
    res, nrec, used, pused, terminal = whole(fmt, a, b, rev, L, combo)
    assert nrec == n and terminal and same(res, want) is None, same(res, want)
    # *consumed: the first byte after the last read line taken -- what follows holds no read
    assert len(tu.read_lines(fmt, a[:used])) == ((n + 1) // 2 if b is not None else n) and (used == len(a) or a[used - 1: used] == b"\n")
    if b is not None:
        assert len(tu.read_lines(fmt, b[:pused])) == n // 2 and (pused == len(b) or b[pused - 1: pused] == b"\n")
    else:
        assert tu.read_lines(fmt, a[used:]) == []
    d = DividedPCLReadsSets(L, *combo)
    for cuts in [tu.piece_cuts(max(len(a), len(b or b"")), p) for p in PIECES] + [list(c) for c in extra_cuts]:
        pc = None if b is None else [min(c, len(b)) for c in cuts[:-1]] + [len(b)]
        ca = [min(c, len(a)) for c in cuts[:-1]] + [len(a)]
        got, m, term, _ = tu.feed(d, fmt, a, b, rev, ca, pc)
        assert m == n and term and same(got, want) is None, (cuts[:3], m, n, same(got, want))
    d.close()
    return n


@pytest.mark.parametrize("L,n", SIZES)
@pytest.mark.parametrize("combo", [SEP_N, N_LQ])
def test_fasta_single_one_header_per_read(tmp_path, L, n, combo):
    a = tu.write_fasta(records(L, n), seed=1)
    assert check_whole_and_pieces(tu.FASTA, a, None, False, L, combo, tmp_path) == n


@pytest.mark.parametrize("L,n", SIZES)
def test_fasta_every_writer_option_and_cuts_by_construction(tmp_path, L, n):
    a = tu.write_fasta(records(L, n), seed=2, crlf=True, trailing_newline=False, comments=True, multi_headers=True, header_last=True, tail_text=True)
    assert a[:1] == b";" and a.endswith(b"\r\n>the end")
    h = a.index(b">r5")                                  # a header line in the middle
    eol = a.index(b"\n", h)
    last = a.rindex(b"\n") + 1                           # the final line, which has no newline
    cuts = [[h + 2, len(a)], [h + 1, len(a)], [eol + 1, len(a)], [last, len(a)], [h + 1, h + 2, eol + 1, last, len(a)]]
    assert check_whole_and_pieces(tu.FASTA, a, None, False, L, SEP_N, tmp_path, cuts) == n
    # the same with the last READ line as the line without a newline
    b = tu.write_fasta(records(L, n), seed=3, trailing_newline=False, multi_headers=True)
    last = b.rindex(b"\n") + 1
    assert check_whole_and_pieces(tu.FASTA, b, None, False, L, N_LQ, tmp_path, [[last, len(b)], [last - 1, last, len(b)]]) == n


@pytest.mark.parametrize("L,n", SIZES)
def test_lines(tmp_path, L, n):
    a = tu.write_lines(records(L, n), crlf=True, trailing_newline=False, tail_text=True)
    last = a.rindex(b"\n") + 1
    assert check_whole_and_pieces(tu.LINES, a, None, False, L, SEP_N, tmp_path, [[last, len(a)]]) == n
    assert check_whole_and_pieces(tu.LINES, tu.write_lines(records(L, n)), None, False, L, N_LQ, tmp_path) == n


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("short", [None, 1, 0])
def test_fasta_pair(tmp_path, rev, short):
    """equal lengths, the second file one read short, the first file one read short: the reference stops at the first
    exhausted file"""
    L, n = 100, 1200
    reads = records(L, n)
    n_a, n_b = n // 2 - (short == 0), n // 2 - (short == 1)
    a = tu.write_fasta(reads[0::2][:n_a], seed=1, comments=True, tail_text=True)
    b = tu.write_fasta(reads[1::2][:n_b], seed=2, crlf=True, multi_headers=True, header_last=True, trailing_newline=False)
    want = 2 * n_a if n_a <= n_b else 2 * n_b + 1
    assert check_whole_and_pieces(tu.FASTA, a, b, rev, L, SEP_N, tmp_path) == want
    if rev:                                               # lower case in the reverse-complemented file is upper-cased by the table
        low = b.replace(reads[1].tobytes(), reads[1].tobytes().lower(), 1)
        assert low != b
        res, nrec, _, _, _ = whole(tu.FASTA, a, low, True, L, SEP_N)
        assert nrec == want and same(res, expected(tu.FASTA, a, b, True, L, SEP_N)[0]) is None


def test_header_only_and_empty_pieces():
    L = 21
    reads = records(L, 300)
    d = DividedPCLReadsSets(L, *SEP_N)
    for fmt, text, final in ((tu.FASTA, b">h1\n;c\r\n>h2\n", False), (tu.FASTA, b">h1\n;c\n>h2", True), (tu.FASTA, b"", True), (tu.FASTA, b"", False),
                             (tu.LINES, b"", True), (tu.LINES, bytes(reads[0][:10]), False), (tu.FASTA, b">h\n" + bytes(reads[0]), False)):
        res, nrec, used, _ = d.divide_text(fmt, text, None, False, final=final)
        assert (nrec, used, res["n_hq"] + res["n_lq"] + res["n_n"]) == (0, 0, 0), (fmt, text)
        assert d.last_was_terminal() == final
    res, nrec, used, pused = d.divide_text(tu.FASTA, b">a\n", b">b\n;\n", False, final=True)
    assert (nrec, used, pused) == (0, 0, 0)
    # everything handed over in a piece that is not the last, then an empty final piece
    a = tu.write_fasta(reads, seed=4)
    res, nrec, used, _ = d.divide_text(tu.FASTA, a, None, False, final=False)
    assert nrec == 300 and used == len(a) and not d.last_was_terminal()
    assert same(res, oracle_divide(np.array(reads), None, *SEP_N)) is None
    res, nrec, used, _ = d.divide_text(tu.FASTA, a[used:], None, False, final=True)
    assert (nrec, used) == (0, 0) and d.last_was_terminal()
    # header lines behind the last read are handed over again: consumed stops in front of them
    t = b">x\n" + bytes(reads[0]) + b"\n>trailing\n;more\n"
    res, nrec, used, _ = d.divide_text(tu.FASTA, t, None, False, final=False)
    assert nrec == 1 and used == 3 + L + 1
    d.close()


def test_refusals_leave_the_divider_usable():
    L, n = 21, 300
    reads = np.array(records(L, n))
    good = tu.write_fasta(reads, seed=5)
    want = oracle_divide(reads, None, *SEP_N)
    row = reads[7].tobytes()

    def edited(new):
        t = good.replace(row + b"\n", new + b"\n", 1)
        assert t != good
        return t
    bad_symbol = bytearray(row)
    bad_symbol[4] = ord("X")
    cases = [("an empty line", tu.FASTA, edited(b""), None, tu.E_PARAM),
             ("a read one symbol longer", tu.FASTA, edited(row + b"A"), None, tu.E_PARAM),
             ("a read one symbol shorter", tu.FASTA, edited(row[:-1]), None, tu.E_PARAM),
             ("a lower-case read", tu.FASTA, edited(row.lower()), None, tu.E_SYMBOL),
             ("a symbol outside ACGNT", tu.FASTA, edited(bytes(bad_symbol)), None, tu.E_SYMBOL),
             ("LINES with a pair", tu.LINES, tu.write_lines(reads), tu.write_lines(reads), tu.E_PARAM),
             ("format 7", 7, good, None, tu.E_PARAM)]
    d = DividedPCLReadsSets(L, *SEP_N)
    for name, fmt, a, b, code in cases:
        if fmt in (tu.FASTA, tu.LINES) and b is None:
            assert tu.restate(fmt, a, b, False, L) == code, name          # the restatement refuses it for the same reason
        with pytest.raises(PgrcMatchError) as e:
            d.divide_text(fmt, a, b, False, final=True)
        assert e.value.code == code, name
        res, nrec, used, _ = d.divide_text(tu.FASTA, good, None, False, final=True)
        assert nrec == n and used == len(good) and same(res, want) is None, name
    with pytest.raises(PgrcMatchError) as e:                               # rev_compl_pair without a pair, one read per line
        d.divide_text(tu.LINES, tu.write_lines(reads), None, True, final=True)
    assert e.value.code == tu.E_PARAM
    d.close()
    q = DividedPCLReadsSets(L, 0.2, False, False, True)                    # a quality division: these formats carry no qualities
    for fmt, text in ((tu.FASTA, good), (tu.LINES, tu.write_lines(reads))):
        with pytest.raises(PgrcMatchError) as e:
            q.divide_text(fmt, text, None, False, final=True)
        assert e.value.code == tu.E_PARAM
    quals = make_records(seed=1, n=n, L=L)[1]
    fq = make_fastq(reads, quals, seed=1)
    res, nrec, _, _ = q.divide_text(tu.FASTQ, fq, None, False, final=True)      # ... and still takes FASTQ
    assert nrec == n and same(res, oracle_divide(reads, quals, 0.2, False, False, True)) is None
    q.close()


@pytest.mark.parametrize("paired", [False, True])
def test_fastq_forwards_to_divide_fastq(paired):
    L, n = 100, 1200
    reads, quals = make_records(seed=11, n=n, L=L)
    a = make_fastq(reads[0::2] if paired else reads, quals[0::2] if paired else quals, seed=1, crlf=True)
    b = make_fastq(reads[1::2], quals[1::2], seed=2, trailing_newline=False) if paired else None
    d = DividedPCLReadsSets(L, *COMBOS[5])
    want = d.divide_fastq(a, b, paired, final=True)
    got = d.divide_text("fastq", a, b, paired, final=True)
    assert got[1:] == want[1:] and got[1] == n and same(got[0], want[0]) is None
    want = d.divide_fastq(a[:5000], b[:5000] if paired else None, paired, final=False)
    got = d.divide_text(tu.FASTQ, a[:5000], b[:5000] if paired else None, paired, final=False)
    assert got[1:] == want[1:] and 0 < got[1] < n and same(got[0], want[0]) is None
    d.close()


@pytest.mark.parametrize("fmt", [tu.FASTA, tu.LINES])
def test_read_sets_take_the_divider_after_a_text_run(fmt):
    """pgrc_rsets_append_divider after a FASTA and after a LINES run: the same rows and mappings as appending the host batch"""
    L, n = 100, 1200
    reads = records(L, n)
    text = tu.write_fasta(reads, seed=6, comments=True) if fmt == tu.FASTA else tu.write_lines(reads, crlf=True)
    div = DividedPCLReadsSets(L, *SEP_N)
    a, b = DividedReadsSets(L, True, False), DividedReadsSets(L, True, False)
    cut = text.index(b"\n", len(text) // 2) + 1
    for piece, final in ((text[:cut], False), (text[cut:], True)):        # two batches: the second one's indexes are shifted
        batch, nrec, used, _ = div.divide_text(fmt, piece, None, False, final=final)
        assert used == len(piece) and nrec > 0 and batch["n_n"] > 0
        a.append_divider(div)
        b.append(batch, nrec)
    a.finish()
    b.finish()
    assert a.info()["reads_total_count"] == n
    assert ru.same_state(ru.device_state(a), ru.device_state(b))
    for s in (a, b, div):
        s.close()


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("two_files", [False, True])
def test_verifier_takes_a_fasta_source(kind, two_files):
    """a decode job verified against its source as FASTA, in two pieces: verdict and counts are those of the same job verified
    against the FASTQ form of the same reads; one read changed is a mismatch, not an error"""
    import verify_util as vu
    from test_gpu_verify import plain_job
    dec, files = plain_job(37, 500, seed=9, two_files=two_files)
    changed = [f.copy() for f in files]
    changed[-1][123, 5] = ord("A") if changed[-1][123, 5] != ord("A") else ord("C")
    for src, ok in ((files, True), (changed, False)):
        fa = [tu.write_fasta(f, seed=k, comments=True, multi_headers=True, header_last=bool(k)) for k, f in enumerate(src)]
        fq = [vu.fastq_text(f, seed=k) for k, f in enumerate(src)]
        with Verifier(dec, kind) as v:
            at, total = [0, 0], 0
            for final in (False, True):
                ends = [len(t) if final else t.index(b"\n", len(t) // 2) + 1 for t in fa]
                used, pused, nrec = v.add_text("fasta", fa[0][at[0]: ends[0]], fa[1][at[1]: ends[1]] if two_files else None, final=final)
                at = [at[0] + used, at[1] + pused]
                total += nrec
            got = v.finish()
        with Verifier(dec, kind) as v:
            assert vu.feed_fastq(v, fq[0], fq[1] if two_files else None, [len(fq[0]) // 2 + 7]) == total
            want = v.finish()
        assert total == sum(f.shape[0] for f in src)
        assert got == want == vu.reference(kind, src, files) and got["ok"] == ok
    with Verifier(dec, kind) as v:                        # refusals come back as the divider's, the handle stays usable
        with pytest.raises(PgrcMatchError) as e:
            v.add_text(7, b"ACGT\n", b"" if two_files else None, final=True)
        assert e.value.code == tu.E_PARAM and "add_text" in str(e.value)
        if two_files:
            with pytest.raises(PgrcMatchError):
                v.add_text("lines", b"ACGT\n", b"ACGT\n", final=True)
        v.add_text("fasta", *[tu.write_fasta(f) for f in files], final=True)
        assert v.finish()["ok"]


# ---- one text path for the three formats: state kept per file must not outlive its run, a refusal must leave what it leaves
# today, and the rule of what a call takes from a pair must be one rule

def fastq_pieces(d, a, b, rev, piece):
    """tests/test_gpu_divide.py's piece loop on a divider that is already in use -> (result, records, terminal, bytes consumed)"""
    parts, buf, at, used_all = [], [b"", b""], [0, 0], [0, 0]
    src = [a, b if b is not None else b""]
    while True:
        for f in range(2 if b is not None else 1):
            buf[f] += src[f][at[f]: at[f] + piece]
            at[f] += piece
        final = at[0] >= len(src[0]) and at[1] >= len(src[1])
        res, nrec, used, pused = d.divide_fastq(buf[0], buf[1] if b is not None else None, rev, final=final)
        parts.append((res, nrec))
        buf[0], buf[1] = buf[0][used:], buf[1][pused:]
        used_all = [used_all[0] + used, used_all[1] + pused]
        if final:
            break
    res, n = tu.concat(parts)
    return res, n, d.last_was_terminal(), used_all


def test_one_divider_takes_the_formats_in_turn():
    """paired FASTQ, FASTA, lines, FASTQ, a FASTA pair of unequal length, FASTA -- on ONE divider, whole and in pieces of 257
    bytes, every file with another number of lines: nothing a run keeps per file (line and read counts, the list of read
    lines, the ends of what was taken, the second file's slots) may reach the next one"""
    L, n = 21, 300
    reads = np.array(records(L, n))
    quals = make_records(seed=5, n=n, L=L)[1]
    combo = SEP_N
    steps = [(tu.FASTQ, make_fastq(reads[0::2], quals[0::2], seed=1), make_fastq(reads[1::2], quals[1::2], seed=2, crlf=True), True, n),
             (tu.FASTA, tu.write_fasta(reads[:280], seed=1, comments=True), None, False, 280),
             (tu.LINES, tu.write_lines(reads[:190], crlf=True, trailing_newline=False), None, False, 190),
             (tu.FASTQ, make_fastq(reads[:250], quals[:250], seed=3, trailing_newline=False), None, False, 250),
             (tu.FASTA, tu.write_fasta(reads[0::2], seed=3, multi_headers=True), tu.write_fasta(reads[1::2][:149], seed=4, crlf=True), True, 299),
             (tu.FASTA, tu.write_fasta(reads, seed=7, multi_headers=True, header_last=True), None, False, n)]
    assert len({len(tu.getlines(s[1])) for s in steps}) == len(steps)
    d = DividedPCLReadsSets(L, *combo)
    for k, (fmt, a, b, rev, want_n) in enumerate(steps):
        if fmt == tu.FASTQ:
            want = oracle_divide_fastq(a, b, rev, L, combo)
        else:
            rows = tu.restate(fmt, a, b, rev, L)
            assert rows.shape[0] == want_n
            want = oracle_divide(rows, None, *combo)
        res, nrec, used, pused = d.divide_text(fmt, a, b, rev, final=True)
        assert nrec == want_n and d.last_was_terminal() and same(res, want) is None, (k, nrec, same(res, want))
        if fmt == tu.FASTQ:
            assert (used, pused) == (len(a), len(b) if b is not None else 0), k
        else:
            assert len(tu.read_lines(fmt, a[:used])) == ((want_n + 1) // 2 if b is not None else want_n), k
            assert used == len(a) or a[used - 1: used] == b"\n", k
            assert tu.read_lines(fmt, a[used:]) == [], k
            if b is not None:
                assert len(tu.read_lines(fmt, b[:pused])) == want_n // 2 and tu.read_lines(fmt, b[pused:]) == [], k
            else:
                assert pused == 0, k
        if fmt == tu.FASTQ:
            got, m, term, used_all = fastq_pieces(d, a, b, rev, 257)
            assert used_all == [len(a), len(b) if b is not None else 0], k
        else:
            cuts = tu.piece_cuts(max(len(a), len(b or b"")), 257)
            got, m, term, _ = tu.feed(d, fmt, a, b, rev, cuts)
        assert m == want_n and term and same(got, want) is None, (k, m, same(got, want))
    d.close()


def appended(div, L, separate_n, n_reads_lq):
    s = DividedReadsSets(L, separate_n, n_reads_lq)
    s.append_divider(div)
    s.finish()
    st = ru.device_state(s)
    s.close()
    return st


def test_a_refusal_leaves_the_last_run_standing_or_not():
    """the refusals of FASTA / one-read-per-line text come before anything of the divider changes: pgrc_rsets_append_divider still
    takes the sets of the good run before them.  A FASTQ call that fails has dropped them: PGRC_E_STATE."""
    L, n = 21, 300
    reads = np.array(records(L, n))
    good = tu.write_fasta(reads, seed=5)
    lines = tu.write_lines(reads)
    div = DividedPCLReadsSets(L, *SEP_N)
    batch, nrec, _, _ = div.divide_text(tu.FASTA, good, None, False, final=True)
    host = DividedReadsSets(L, True, False)
    host.append(batch, nrec)
    host.finish()
    want = ru.device_state(host)
    host.close()
    assert want["A"] == n and ru.same_state(appended(div, L, True, False), want)
    for name, fmt, a, b, rev in (("format 7", 7, good, None, False), ("lines with a pair", tu.LINES, lines, lines, False),
                                 ("lines with rev_compl_pair", tu.LINES, lines, None, True)):
        with pytest.raises(PgrcMatchError) as e:
            div.divide_text(fmt, a, b, rev, final=True)
        assert e.value.code == tu.E_PARAM, name
        assert ru.same_state(appended(div, L, True, False), want), name
    # a quality division: its good run is FASTQ, and a FASTA or lines file of two records is refused
    qcombo = (0.2, False, True, False)
    quals = make_records(seed=1, n=n, L=L)[1]
    fq = make_fastq(reads, quals, seed=1)
    q = DividedPCLReadsSets(L, *qcombo)
    batch, nrec, _, _ = q.divide_fastq(fq, None, False, final=True)
    host = DividedReadsSets(L, True, False)
    host.append(batch, nrec)
    host.finish()
    qwant = ru.device_state(host)
    host.close()
    for fmt, text in ((tu.FASTA, tu.write_fasta(reads[:2])), (tu.LINES, tu.write_lines(reads[:2]))):
        with pytest.raises(PgrcMatchError) as e:
            q.divide_text(fmt, text, None, False, final=True)
        assert e.value.code == tu.E_PARAM
        assert ru.same_state(appended(q, L, True, False), qwant), fmt
    # FASTQ text that ends inside a record: the call has dropped the last run's sets before it fails, through either entry
    cut = fq[: fq.rstrip(b"\n").rfind(b"\n+")]
    for entry in (lambda: q.divide_fastq(cut, None, False, final=True), lambda: q.divide_text(tu.FASTQ, cut, None, False, final=True)):
        q.divide_fastq(fq, None, False, final=True)
        with pytest.raises(PgrcMatchError) as e:
            entry()
        assert e.value.code == tu.E_PARAM and "ends inside a record" in str(e.value)
        with pytest.raises(PgrcMatchError) as e:
            appended(q, L, True, False)
        assert e.value.code == 6                             # PGRC_E_STATE
    for s in (div, q):
        s.close()


# (records of the first file, of the second, calls as (records handed over so far of the first, of the second, final bits),
#  records each call takes, the call that is terminal): worked out from the reference's iteration -- the two files in turn,
#  first file first, until the one whose turn it is has no more; a call takes the whole pairs it holds, and the odd last read
#  once the second file is known to have no mate for it
TAKE_CASES = {
    "3 against 5, the first ends": (3, 5, [(3, 5, 2)], [6], 0),
    "3 against 5, the second ends, the first goes on": (6, 5, [(3, 5, 4), (6, 5, 1)], [6, 5], 1),
    "5 against 3, the first ends, the second goes on": (5, 6, [(5, 3, 2), (5, 6, 1)], [6, 4], 1),
    "5 against 3, the second ends": (5, 3, [(5, 3, 4)], [7], 0),
    "the first is through, its mates arrive later": (3, 5, [(3, 1, 2), (3, 5, 2)], [2, 4], 1),
    "the second is through, the first's reads arrive later": (5, 3, [(1, 3, 4), (5, 3, 4)], [2, 5], 1),
    "neither is through, then the first ends": (3, 5, [(2, 4, 0), (3, 5, 2)], [4, 2], 1),
}


@pytest.mark.parametrize("case", list(TAKE_CASES))
def test_fastq_and_fasta_pairs_take_the_same_records(case):
    """what a call takes from a pair and whether it is the terminal one depends on the numbers of records alone: the same
    calls in FASTQ and in FASTA give the same counts, the same terminal call and the same rows"""
    L = 21
    na, nb, calls, want_nrec, want_terminal = TAKE_CASES[case]
    reads = np.array(records(L, 300))
    quals = make_records(seed=5, n=300, L=L)[1]
    ra, rb = reads[0:2 * na:2], reads[1:2 * nb:2]
    qa, qb = quals[0:2 * na:2], quals[1:2 * nb:2]
    texts = {tu.FASTQ: ([make_fastq(ra[i:i + 1], qa[i:i + 1], seed=i) for i in range(na)],
                        [make_fastq(rb[i:i + 1], qb[i:i + 1], seed=50 + i, crlf=True) for i in range(nb)]),
             tu.FASTA: ([tu.write_fasta(ra[i:i + 1], seed=i, comments=True) for i in range(na)],
                        [tu.write_fasta(rb[i:i + 1], seed=50 + i, crlf=True) for i in range(nb)])}
    rows = tu.restate(tu.FASTA, b"".join(texts[tu.FASTA][0]), b"".join(texts[tu.FASTA][1]), True, L)
    assert rows.shape[0] == sum(want_nrec)
    want = oracle_divide(rows, None, *SEP_N)
    seen = {}
    for fmt, (ta, tb) in texts.items():
        d = DividedPCLReadsSets(L, *SEP_N)
        at, parts, terminal = [0, 0], [], []
        for ha, hb, bits in calls:
            a, b = b"".join(ta[:ha]), b"".join(tb[:hb])
            res, nrec, used, pused = d.divide_text(fmt, a[at[0]:], b[at[1]:], True, final=bits)
            parts.append((res, nrec))
            terminal.append(d.last_was_terminal())
            at = [at[0] + used, at[1] + pused]
        d.close()
        got, total = tu.concat(parts)
        assert same(got, want) is None, (fmt, same(got, want))
        seen[fmt] = ([p[1] for p in parts], terminal.index(True) if True in terminal else None)
        assert terminal.count(True) == 1 and terminal[-1]
    assert seen[tu.FASTQ] == seen[tu.FASTA] == (want_nrec, want_terminal)
