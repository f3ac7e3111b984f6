"""The two index sets of a context (pgrc_amd/csrc/ctx.h, PgrcIndexSet) through sequences of calls that build, keep, serve
and give up either of them: one context is walked from the dual kernel through exports, single passes, a prepared pair,
the screened schedule and the out-of-memory retreat, and after every step the results equal the oracle's and every
exported index the oracle's index of that strand, byte for byte.  Public MatchContext calls only."""
import numpy as np
import pytest

import oracle as orc
from util import assert_same_results, make_inputs, pack_rows, revcomp

pytestmark = pytest.mark.gpu

N_WITH_N = 100


@pytest.fixture(scope="module")
def case():
    pg, reads = make_inputs(300_000, 6_000, 150, seed=38, n_with_n=N_WITH_N)
    index = [orc.oracle_index(pg, 38)[1:], orc.oracle_index(revcomp(pg), 38)[1:]]
    return {"pg": pg, "reads": reads, "index": index, "o": orc.oracle_match("c", pg, reads, 38, 3, 0),
            "o5": orc.oracle_match("c", pg, reads[:5000], 38, 3, 0)}


def _results(ctx):
    pos, rc, mism, hist, matched = ctx.get_results()
    return {"pos": pos, "rc": rc, "mism": mism, "hist": hist, "matched": matched}


def _fresh_run(ctx, want, what, passes=None):
    ctx.init_results()
    if passes is None:
        ctx.run(True)
    else:
        for strand in passes:
            ctx.run_pass(strand)
    assert_same_results(_results(ctx), want, what)


def _export(ctx, case, strand, what):
    cumm, positions = ctx.export_index(strand)
    assert np.array_equal(cumm, case["index"][strand][0]), f"{what}: cumm of strand {strand}"
    assert np.array_equal(positions, case["index"][strand][1]), f"{what}: positions of strand {strand}"


def test_one_context_through_every_use_of_its_index_sets(monkeypatch, case):
    from pgrc_amd import MatchContext
    for knob in ("PGRC_DUAL", "PGRC_SCREEN", "PGRC_TEST_NO_SECOND_INDEX"):
        monkeypatch.delenv(knob, raising=False)
    ctx = MatchContext(150, 38, 3, 0, "c")
    ctx.set_pg_ascii(case["pg"])
    ctx.set_reads_ascii(case["reads"])
    # 1. the dual kernel: both sets built
    _fresh_run(ctx, case["o"], "1: dual run")
    assert ctx.counters()["screened"] == 2
    # 2. exports of either strand, in an order that leaves and comes back to a strand
    for strand in (0, 1, 0):
        _export(ctx, case, strand, "2: after the dual run")
    # 3. the same run behind the exports
    _fresh_run(ctx, case["o"], "3: dual run after exports")
    assert ctx.counters()["screened"] == 2
    # 4. one pass per strand, each building its index
    _fresh_run(ctx, case["o"], "4: run_pass(0), run_pass(1)", passes=(0, 1))
    # 5. a pair built ahead, an export between it and the run it was built for
    ctx.prepare_index(True)
    _export(ctx, case, 0, "5: after prepare_index")
    _fresh_run(ctx, case["o"], "5: run after prepare_index and an export")
    assert ctx.counters()["screened"] == 2
    # 6. the screened schedule: three launches that each name their strand
    monkeypatch.setenv("PGRC_SCREEN", "1")
    ctx.reload_options()
    _fresh_run(ctx, case["o"], "6: screened run")
    assert ctx.counters()["screened"] == 1
    monkeypatch.delenv("PGRC_SCREEN")
    ctx.reload_options()
    # 7. the second set "does not fit" on a context that holds two populated sets: the retreat, then the two passes
    monkeypatch.setenv("PGRC_TEST_NO_SECOND_INDEX", "1")
    ctx.reload_options()
    _fresh_run(ctx, case["o"], "7: run without room for the second set")
    assert ctx.counters()["schedule_downgraded"] == 1 and ctx.counters()["screened"] == 0
    _export(ctx, case, 1, "7: after the retreat")
    monkeypatch.delenv("PGRC_TEST_NO_SECOND_INDEX")
    ctx.reload_options()
    ctx.set_reads_ascii(case["reads"][:5000])              # another read set: the two-index schedule is tried again
    _fresh_run(ctx, case["o5"], "7: another read set after the retreat")
    assert ctx.counters()["screened"] == 2 and ctx.counters()["schedule_downgraded"] == 0


def test_streamed_two_passes_find_each_strands_index(monkeypatch, case):
    """PGRC_DUAL=0: every block of a streamed run takes the forward pass and then the RC pass, each on its own index set."""
    from pgrc_amd import MatchContext
    monkeypatch.setenv("PGRC_DUAL", "0")
    reads = case["reads"]
    n_lq = reads.shape[0] - N_WITH_N
    sets = [(pack_rows(reads[:n_lq]), n_lq, 4), (pack_rows(reads[n_lq:], b"ACGNT"), N_WITH_N, 5)]
    ctx = MatchContext(150, 38, 3, 0, "c")
    ctx.set_pg_ascii(case["pg"])
    for prepare in (False, True):
        if prepare:
            ctx.prepare_index(True)
        pos, rc, mism, hist, matched = ctx.match_streamed(sets, blocks=3)
        got = {"pos": pos, "rc": rc, "mism": mism, "hist": hist, "matched": matched}
        assert_same_results(got, case["o"], f"streamed two passes, prepare_index={prepare}")
        assert_same_results(_results(ctx), case["o"], f"streamed two passes, prepare_index={prepare}: results on the device")
        assert ctx.counters()["screened"] == 0
