"""The parallel form of markAndRemoveExactMatches that pgmap.hip runs (tests/pgmap_par_util.py: threshold rule, next
pointers by prefix maximum, path by pointer jumping, mark positions, both streams, the text by binary search) against the
literal loop (pgmap_util.mark_and_remove): on every part of the reference-made fixtures and on hand-made match lists in all
four (dest_is_src, rev_compl) settings.  No GPU."""
import os

import numpy as np
import pytest

import pgmap_par_util as pp
import pgmap_util as pu
from test_pgmap_oracle import FIXTURES, load_case

ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[6:-4])
def test_fixture_parts(path):
    z, texts, tl = load_case(path)
    hq = texts[0]
    if hq.size < tl:
        # no matcher for this fixture: the caller's case (the texts as they are, no streams), nothing for the parallel form
        assert all(z[f"mapped{p}"].tobytes() == texts[p].tobytes() and z[f"off{p}"].size == 0 for p in range(3))
        return
    trimmed_out = 0
    for p, dest in enumerate(texts):
        got = pp.mark_and_remove_parallel(dest, z[f"matches{p}"], p == 0, True, tl, hq.size, detail=True)
        for k, g in zip(("mapped", "off", "len"), got[:3]):
            assert g == z[f"{k}{p}"].tobytes(), f"part {p}: {k} differs from the reference's"
        d = got[3]
        assert np.array_equal(d["kept"], pp.greedy_kept(d["e"], tl))
        trimmed_out += int((~d["kept"] & ~d["dead"]).sum())
    if "low_complexity" in path:
        assert trimmed_out > 0                              # matches that the trimming left shorter than min_len


def _brute_next(e, t):
    n = e.size
    out = np.full(n, n, dtype=np.int64)
    for i in range(n):
        later = np.flatnonzero(t[i + 1:] >= e[i])
        if later.size:
            out[i] = i + 1 + later[0]
    return out


SETTINGS = [(False, False), (False, True), (True, False), (True, True)]


@pytest.mark.parametrize("dest_is_src,rev_compl", SETTINGS)
def test_hand_made_lists(dest_is_src, rev_compl):
    rng = np.random.default_rng(100 + 2 * dest_is_src + rev_compl)
    seen = {"dup": 0, "short_after_margin": 0, "src_eq_dst": 0, "mark_at_0": 0, "mark_to_end": 0, "adjacent": 0, "dead": 0, "trimmed_out": 0}
    for case in range(90):                                  # 4 x 90 = 360 lists
        min_len = int(rng.integers(1, 40))
        n2 = int(rng.integers(8 * min_len + 8, 3000))
        src_len = n2 if dest_is_src else int(rng.integers(4 * min_len + 8, 3000))
        count = int(rng.integers(0, 60)) if case % 10 else 0
        m = pp.random_case(rng, n2, src_len, count, min_len, dest_is_src, rev_compl) if case % 10 else np.zeros((0, 3), np.uint64)
        dest = ACGT[rng.integers(0, 4, size=n2)]
        want = pu.mark_and_remove(dest, m, dest_is_src, rev_compl, min_len, src_len)
        mapped, off, lens, d = pp.mark_and_remove_parallel(dest, m, dest_is_src, rev_compl, min_len, src_len, detail=True)
        assert (mapped, off, lens) == want, (case, "parallel form differs from the loop")
        # the steps, one by one
        assert np.array_equal(d["kept"], pp.greedy_kept(d["e"], min_len)), case
        live = ~d["dead"]
        assert np.array_equal(d["next"][live], _brute_next(d["e"], d["t"])[live]), case
        assert not (d["kept"] & d["dead"]).any()
        assert d["passes"] <= max(0, int(np.ceil(np.log2(max(1, d["e"].size)))))
        assert np.array_equal(np.flatnonzero(np.frombuffer(mapped, np.uint8) == pu.MATCH_MARK), d["mp"])
        # what the lists hold
        nd, ns, nl = pp.normalise(m, n2, dest_is_src, rev_compl)
        seen["dup"] += int(m.shape[0] > d["unique"])
        if dest_is_src and rev_compl:
            seen["short_after_margin"] += int(((nl < min_len) & (m[:, 1].astype(np.int64) >= min_len)).any())
        mi = m.astype(np.int64)
        seen["src_eq_dst"] += int(((n2 - (mi[:, 2] + mi[:, 1]) if rev_compl else mi[:, 2]) == mi[:, 0]).any())   # (before the margin)
        seen["mark_at_0"] += int(mapped[:1] == b"%")
        seen["mark_to_end"] += int(mapped[-1:] == b"%" and d["dp"].size and d["dp"][-1] + d["lp"][-1] == n2)
        seen["adjacent"] += int(b"%%" in mapped)
        seen["dead"] += int(d["dead"].any())
        seen["trimmed_out"] += int((~d["kept"] & live).any())
    for k, v in seen.items():
        if k == "short_after_margin" and not (dest_is_src and rev_compl):
            continue
        if k == "src_eq_dst" and not dest_is_src:
            continue
        if k == "mark_at_0" and dest_is_src and rev_compl:      # (the collision margin moves a match at 0 off it)
            continue
        assert v > 0, f"no list with {k}"


def test_frugal_widths_and_layout():
    vals = np.array([0, 127, 128, 16383, 16384, 2**21 - 1, 2**21, 2**63, 2**64 - 1], dtype=np.uint64)
    assert pp.frugal_widths(vals).tolist() == [1, 1, 2, 2, 3, 3, 4, 10, 10]
    sp = np.arange(vals.size, dtype=np.int64)
    off, lens = pp.streams(sp[:7], vals[:7].astype(np.int64) + 50, 50, 10)
    assert lens == pu.frugal_stream([50] + vals[:7].tolist())
    assert pp.streams(sp[:2], np.array([60, 61]), 50, 2**32)[0] == (0).to_bytes(8, "little") + (1).to_bytes(8, "little")
    assert len(off) == 7 * 4
