"""The Pg-vs-Pg matcher's context (memctx.h) across calls: what one call leaves in the context must not reach the next.

One context runs a sequence of calls that between them take every route of the match (host / device destination, the source
as its own destination, with and without N, no window at all, a refusal in the middle, the probe's regrow-and-rerun, growing
buffers), and after every step the matches equal the oracle's (and the compiled reference's where it is built), equal what a
context made for that step alone finds, and map (pgrc_mem_mark_and_remove) to what tests/pgmap_util.py makes of them.  The
per-event arrays of the match are reused under several meanings from phase to phase and from call to call: a phase that read
what an earlier call left there would show here.  Then every refusal and forwarded failure of the two files by code and exact
text, each followed by a good call on the same context, and the create / destroy pairs that run no match.

Sizes: a source of 30 000 symbols, destinations of 0 to 3 000.  A destination is one staging chunk, the probe a few blocks,
the event and run arrays far below any tile boundary; every path named above still runs."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as orc
import pgmap_util as pu
import varlen_util as vu
from mem_util import make_pair
from pgrc_amd import CopMEMMatcher, PgrcMatchError, VarLenDNACoder, _lib

pytestmark = pytest.mark.gpu

E_PARAM, E_SEED_SHORT, E_SYMBOL, E_STATE = 1, 2, 5, 6
TARGET = 45
HAVE_REF = orc.have_ref() and hasattr(orc.ref(), "pgrc_ref_mem_match")
NO_MATCHES = np.zeros((0, 3), np.uint64)


def dev(text):
    """the text in device memory -> (the tensor, to be kept alive; its address)"""
    t = torch.from_numpy(np.ascontiguousarray(text, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr()


def last_error(m):
    return (_lib.lib.pgrc_mem_last_error(m._h if m is not None else None) or b"").decode()


def set_src_host(m, text):
    """pgrc_mem_set_src_ascii on an existing context (the wrapper only calls it from its constructor)"""
    m._src = np.ascontiguousarray(text, dtype=np.uint8)
    m._ck(_lib.lib.pgrc_mem_set_src_ascii(m._h, m._src.ctypes.data_as(C.c_void_p), m._src.size))


@pytest.fixture(scope="module")
def texts():
    src, small = make_pair(0, G=30000, G2=1500)
    _, small_n = make_pair(0, G=30000, G2=1500, with_n=True)
    _, big = make_pair(0, G=30000, G2=3000)
    assert src.size == 30000 and ord("N") in small_n
    bad = small.copy()
    bad[700] = ord("%")
    return {"src": src, "small": small, "small_n": small_n, "big": big, "short": small[100:120].copy(), "empty": np.zeros(0, np.uint8), "bad": bad}


# (name, destination, dest_is_src, rev_compl, device route); the destination is the text being mapped, in its forward orientation
STEPS = [("host destination, reverse complement", "small", False, True, False),
         ("the source as destination, reverse complement", "src", True, True, False),
         ("device destination, forward, with N", "small_n", False, False, True),
         ("a destination shorter than K", "short", False, True, False),
         ("a destination of length 0", "empty", False, True, False),
         ("a byte outside ACGNT", "bad", False, True, False),
         ("the first call again", "small", False, True, False),
         ("a destination twice as long", "big", False, True, False)]


@pytest.fixture(scope="module")
def expected(texts):
    """per step: the oracle's matches (held to the compiled reference where there is one) and the mapping of them; made once"""
    src, out = texts["src"], {}
    for name, key, dest_is_src, rev_compl, _ in STEPS:
        if key == "bad" or (key, dest_is_src, rev_compl) in out:
            continue
        fwd = texts[key]
        d = orc.mem_dest(src, fwd, dest_is_src, rev_compl)
        want = orc.oracle_mem_match(src, d, dest_is_src, rev_compl, TARGET)
        if HAVE_REF:
            assert np.array_equal(want, orc.ref_mem_match(src, d, dest_is_src, rev_compl, TARGET)), name
        out[(key, dest_is_src, rev_compl)] = (want, pu.mark_and_remove(fwd, want, dest_is_src, rev_compl, TARGET, src.size))
    assert all(len(out[k][0]) > 5 for k in out if k[0] not in ("short", "empty"))
    return out


def unique_count(matches, n2, dest_is_src, rev_compl):
    """distinct matches after the two corrections of markAndRemoveExactMatches (SimplePgMatcher.cpp:58-61, :157-171)"""
    m = np.asarray(matches, dtype=np.int64).reshape(-1, 3)
    s, ln, d = m[:, 0].copy(), m[:, 1].copy(), m[:, 2].copy()
    if rev_compl:
        d = n2 - (d + ln)
    if dest_is_src:
        s, d = np.minimum(s, d), np.maximum(s, d)
        if rev_compl:
            margin = np.where(s + ln > d, (s + ln - d + 1) // 2, 0)
            ln, d = ln - margin, d + margin
    return np.unique(np.stack([d, s, ln], axis=1), axis=0).shape[0] if m.shape[0] else 0


def run_step(m, texts, step):
    """the step's match on context m -> the matches"""
    name, key, dest_is_src, rev_compl, on_device = step
    fwd = texts[key]
    if on_device:
        keep, ptr = dev(fwd)
        return m.matchTextsDevice(ptr, fwd.size, dest_is_src, rev_compl)
    return m.matchTexts(orc.mem_dest(texts["src"], fwd, dest_is_src, rev_compl), dest_is_src, rev_compl)


def check_mapping(m, texts, step, matches, want_map):
    name, key, dest_is_src, rev_compl, _ = step
    fwd = texts[key]
    mapped, off, lens, info = m.markAndRemoveExactMatches(matches)
    assert mapped.tobytes() == want_map[0], f"{name}: mapped text"
    assert off.tobytes() == want_map[1], f"{name}: offsets stream"
    assert lens.tobytes() == want_map[2], f"{name}: lengths stream"
    marks = want_map[0].count(b"%")
    assert info["marks"] == marks and info["matched_symbols"] == fwd.size - len(want_map[0]) + marks, (name, info)
    assert info["unique_matches"] == unique_count(matches, fwd.size, dest_is_src, rev_compl), (name, info)


@pytest.mark.parametrize("event_cap", [None, 7])
def test_one_context_through_a_sequence(texts, expected, monkeypatch, event_cap):
    """The options are read when a context is made, so PGRC_MEM_EVENT_CAP=7 holds for every call of a context made under it:
    with it the whole sequence takes the probe's regrow-and-rerun path (7 events of room, then what the probe counted) and is
    held to fresh contexts that take the plain one; without it the sequence runs as a caller's would."""
    if event_cap:
        monkeypatch.setenv("PGRC_MEM_EVENT_CAP", str(event_cap))
    m = CopMEMMatcher(texts["src"], TARGET, device=0)
    monkeypatch.delenv("PGRC_MEM_EVENT_CAP", raising=False)
    grown = 0
    for step in STEPS:
        name, key, dest_is_src, rev_compl, _ = step
        if key == "bad":
            with pytest.raises(PgrcMatchError) as e:
                run_step(m, texts, step)
            assert e.value.code == E_SYMBOL and last_error(m) == "destination text contains a symbol outside ACGNT"
            with pytest.raises(PgrcMatchError) as e:            # (a failed call leaves nothing to map)
                m.markAndRemoveExactMatches(NO_MATCHES)
            assert e.value.code == E_STATE
            continue
        want, want_map = expected[(key, dest_is_src, rev_compl)]
        got = run_step(m, texts, step)
        assert np.array_equal(got, want), f"{name}: {len(got)} / {len(want)} matches"
        fresh = CopMEMMatcher(texts["src"], TARGET, device=0)
        alone = run_step(fresh, texts, step)
        assert np.array_equal(got, alone), f"{name}: differs from a fresh context's"
        check_mapping(fresh, texts, step, alone, want_map)
        fresh.close()
        check_mapping(m, texts, step, got, want_map)
        grown = max(grown, m.counters()["events"])
    assert grown > 7                                             # (more events than the knob's 7: with it set, the first guess was too small)
    m.close()


# ---------------------------------------------------------------------------------------------- refusals
def refused(m, code, text, call, *args):
    with pytest.raises(PgrcMatchError) as e:
        call(*args)
    assert e.value.code == code, (e.value.code, str(e.value))
    assert last_error(m) == text


@pytest.fixture(scope="module")
def coder():
    for _, _, streams in vu.load_fixtures():
        if 0 in streams:
            c = VarLenDNACoder(vu.parse_stream(streams[0])[2].raw + b"\0", device=0)
            yield c
            c.close()
            return
    raise KeyError("no fixture coded with book 0")


def test_every_refusal_by_code_and_text(texts, expected, coder):
    src, small = texts["src"], texts["small"]
    d = orc.revcomp_ascii(small)
    want, want_map = expected[("small", False, True)]
    keep_s, ps = dev(src)
    keep_o, po = dev(small)

    def good(m):
        got = m.matchTexts(d, False, True)
        assert np.array_equal(got, want)
        check_mapping(m, texts, STEPS[0], got, want_map)

    m = CopMEMMatcher(None, TARGET, device=0)
    refused(m, E_STATE, "match_texts: set the source text first", m.matchTexts, d, False, True)
    refused(m, E_STATE, "match_texts: set the source text first", m.matchTextsDevice, po, small.size, False, True)
    set_src_host(m, src)
    good(m)

    # the source must be over ACGT, through both routes; the context has no source afterwards
    bad_src = src.copy()
    bad_src[777] = ord("N")
    keep_b, pb = dev(bad_src)
    refused(m, E_SYMBOL, "pseudogenome contains a symbol outside ACGT", set_src_host, m, bad_src)
    refused(m, E_STATE, "match_texts: set the source text first", m.matchTexts, d, False, True)
    set_src_host(m, src)
    good(m)
    refused(m, E_SYMBOL, "pseudogenome contains a symbol outside ACGT", m.setSrcDevice, pb, bad_src.size)
    refused(m, E_STATE, "match_texts: set the source text first", m.matchTexts, d, False, True)
    m.setSrcDevice(ps, src.size)
    good(m)
    refused(m, E_PARAM, "set_src_device: the text is not memory of the context's device", m.setSrcDevice, src.ctypes.data, src.size)
    m.setSrcDevice(ps, src.size)
    good(m)

    refused(m, E_PARAM, "Minimal matching length cannot be smaller than K", m.matchTexts, d, False, True, 20)
    good(m)
    refused(m, E_PARAM, "match_texts: dest_is_src with a text of another length", m.matchTexts, d, True, True)
    good(m)
    refused(m, E_PARAM, "match_texts_device: the destination is not memory of the context's device", m.matchTextsDevice, small.ctypes.data, small.size, False, True)
    refused(m, E_STATE, "mark_and_remove: no destination (call pgrc_mem_match_texts first)", m.markAndRemoveExactMatches, want)
    good(m)

    refused(m, E_PARAM, "mark_and_remove: min_match_len is 0", m.markAndRemoveExactMatches, want, 0)
    good(m)
    refused(m, E_PARAM, "mark_and_remove: mapped_out is smaller than the destination", m.markAndRemoveExactMatches, want, None, np.empty(small.size - 1, np.uint8))
    good(m)
    past_src = np.array([[src.size - 10, 50, 0]], np.uint64)
    refused(m, E_PARAM, "mark_and_remove: a match reaches past the source's end", m.markAndRemoveExactMatches, past_src)
    good(m)
    past_dest = np.array([[0, 50, small.size - 10]], np.uint64)
    refused(m, E_PARAM, "mark_and_remove: a match reaches past the destination's end", m.markAndRemoveExactMatches, past_dest)
    good(m)
    refused(m, E_PARAM, "mark_and_remove_resident: part must be 0 (HQ), 1 (LQ) or 2 (N)", m.markAndRemoveExactMatchesResident, want, 3)
    good(m)
    refused(m, E_STATE, "encode_mapped: no resident HQ or LQ text (call pgrc_mem_mark_and_remove_resident for parts 1, 2 and 0 first)", m.encodeMapped, coder)
    good(m)
    m.close()

    for length, code, text in ((20, E_SEED_SHORT, "Minimal matching length too short"), (300, E_PARAM, "target match length above 255 is not supported")):
        with pytest.raises(PgrcMatchError) as e:
            CopMEMMatcher(None, length, device=0)
        assert e.value.code == code and last_error(None) == text


def test_create_and_destroy_without_a_match(texts):
    m = CopMEMMatcher(None, TARGET, device=0)                    # never got a source
    m.close()
    m = CopMEMMatcher(texts["src"], TARGET, device=0)            # its last call failed
    with pytest.raises(PgrcMatchError):
        m.matchTexts(texts["bad"], False, False)
    m.close()
    m = CopMEMMatcher(None, TARGET, device=0)                    # ... and that call was its only one
    with pytest.raises(PgrcMatchError):
        m.matchTexts(texts["small"], False, False)
    m.close()
