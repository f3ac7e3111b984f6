"""The phase times and work counters of a run (pgrc_match_counters) under every schedule that pgrc_match_run and
pgrc_match_run_pass can take: which ms_* fields a schedule fills, which stay exactly 0, that ms_other is the rest of
ms_total, that a single pass does not pick up an event of the run before it, and that every counter word comes from its
own place in the device counter block.  Public MatchContext calls only; the knobs are set in the environment before a
context is made (a context reads them once).

Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

import oracle as orc
from util import assert_same_results, make_inputs

pytestmark = pytest.mark.gpu

N_WITH_N = 100
KNOBS = ("PGRC_DUAL", "PGRC_SCREEN", "PGRC_BUILD_STREAMS", "PGRC_TEST_NO_SECOND_INDEX", "PGRC_EARLY_STOP", "PGRC_HEAD_PAIR",
         "PGRC_NREAD_INLINE", "PGRC_ROUND_SKIP", "PGRC_DUAL_PACK")
TIMES = ("ms_index0", "ms_index1", "ms_match0", "ms_match1", "ms_screen")
DUAL = {"PGRC_DUAL": None}
IN_TURN = {"PGRC_BUILD_STREAMS": "1"}
SCREEN = {"PGRC_DUAL": "0", "PGRC_SCREEN": "1"}
PLAIN = {"PGRC_DUAL": "0", "PGRC_SCREEN": "0"}
NO_ROOM = {"PGRC_TEST_NO_SECOND_INDEX": "1"}


@pytest.fixture(scope="module")
def case():
    pg, reads = make_inputs(300_000, 6_000, 150, seed=38, n_with_n=N_WITH_N)
    return {"pg": pg, "reads": reads, "o": orc.oracle_match("c", pg, reads, 38, 3, 0)}


def _context(knobs, pg, reads, mode="c", L=150, kmax=3):
    from pgrc_amd import MatchContext
    with pytest.MonkeyPatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        for k, v in knobs.items():
            if v is not None:
                mp.setenv(k, v)
        ctx = MatchContext(L, 38, kmax, 0, mode)
    ctx.set_profiling(True)
    ctx.set_pg_ascii(pg)
    ctx.set_reads_ascii(reads)
    return ctx


def _results(ctx):
    pos, rc, mism, hist, matched = ctx.get_results()
    return {"pos": pos, "rc": rc, "mism": mism, "hist": hist, "matched": matched}


def _run(ctx, want, what, passes=None):
    """A run from fresh results; its counters, after the results were held to the oracle's."""
    ctx.init_results()
    if passes is None:
        ctx.run(True)
    else:
        for strand in passes:
            ctx.run_pass(strand)
    assert_same_results(_results(ctx), want, what)
    return ctx.counters()


def _times(c):
    return {"ms_index0": c["ms_index"][0], "ms_index1": c["ms_index"][1], "ms_match0": c["ms_match"][0], "ms_match1": c["ms_match"][1],
            "ms_screen": c["ms_screen"]}


def _check_times(c, what, filled, spans=()):
    """filled: > 0.  spans: between two events that follow each other at once, or a wait: >= 0, the leg says more.
    Every other field: exactly 0."""
    t = _times(c)
    print(f"\n{what}: ms_total {c['ms_total']!r} ms_other {c['ms_other']!r} {t!r}")
    assert c["ms_total"] > 0, what
    for k in TIMES:
        if k in filled:
            assert t[k] > 0, (what, k, t[k])
        elif k in spans:
            assert t[k] >= 0, (what, k, t[k])
        else:
            assert t[k] == 0.0, (what, k, t[k])
    rest = c["ms_total"] - sum(t[k] for k in TIMES)
    assert abs(c["ms_other"] - rest) <= 1e-4 * c["ms_total"] + 1e-4, (what, c["ms_other"], rest)


@pytest.fixture(scope="module")
def dual_run(case):
    ctx = _context(DUAL, case["pg"], case["reads"])
    return ctx, _run(ctx, case["o"], "1: dual, two build streams")


@pytest.fixture(scope="module")
def screen_run(case):
    ctx = _context(SCREEN, case["pg"], case["reads"])
    return ctx, _run(ctx, case["o"], "3: screened")


@pytest.fixture(scope="module")
def plain_run(case):
    ctx = _context(PLAIN, case["pg"], case["reads"])
    return ctx, _run(ctx, case["o"], "4: plain passes")


def test_dual_two_build_streams(dual_run):
    """ms_index[0] is the pair of builds; ms_match[0] is what the reads with N took beyond the dual kernel (two events on
    the main stream, whatever the side stream did between them)."""
    c = dual_run[1]
    _check_times(c, "1: dual, two build streams", ("ms_index0", "ms_screen"), spans=("ms_index1", "ms_match0"))
    assert c["ms_index"][1] < c["ms_index"][0]
    assert c["ms_match"][1] == 0
    assert c["screened"] == 2


def test_dual_builds_in_turn(case):
    c = _run(_context(IN_TURN, case["pg"], case["reads"]), case["o"], "2: dual, builds in turn")
    _check_times(c, "2: dual, builds in turn", ("ms_index0", "ms_index1", "ms_screen"), spans=("ms_match0",))
    assert c["screened"] == 2


def test_screened(screen_run):
    c = screen_run[1]
    _check_times(c, "3: screened", ("ms_index0", "ms_screen", "ms_match0", "ms_match1"))
    assert c["screened"] == 1


def test_plain_passes_and_single_passes(case, plain_run):
    ctx, c = plain_run
    _check_times(c, "4: plain passes", ("ms_index0", "ms_index1", "ms_match0", "ms_match1"))
    assert c["ms_screen"] == 0 and c["screened"] == 0
    # 5. one pass per call on the same context: the other strand's events are those of the run before -- they are not read
    ctx.init_results()
    ctx.run_pass(0)
    _check_times(ctx.counters(), "5: run_pass(0)", ("ms_index0", "ms_match0"))
    ctx.run_pass(1)
    _check_times(ctx.counters(), "5: run_pass(1)", ("ms_index1", "ms_match1"))
    assert_same_results(_results(ctx), case["o"], "5: run_pass(0), run_pass(1)")


def test_no_room_for_the_second_index(case):
    c = _run(_context(NO_ROOM, case["pg"], case["reads"]), case["o"], "6: fallback")
    _check_times(c, "6: fallback", ("ms_index0", "ms_index1", "ms_match0", "ms_match1"))
    assert c["ms_screen"] == 0 and c["schedule_downgraded"] == 1


def test_prepared_indexes(case, dual_run):
    ctx = _context(DUAL, case["pg"], case["reads"])
    ctx.prepare_index(True)
    c = _run(ctx, case["o"], "7: prepared indexes")
    _check_times(c, "7: prepared indexes", ("ms_screen",), spans=("ms_index0", "ms_index1", "ms_match0"))
    built = dual_run[1]["ms_index"][0]
    assert c["ms_index"][0] < built and c["ms_index"][1] < built      # waits, not builds
    assert c["screened"] == 2


def test_mode_d_has_the_total_only():
    pg, reads = make_inputs(100_000, 2_000, 100, seed=3)
    c = _run(_context({}, pg, reads, mode="d", L=100, kmax=2), orc.oracle_match("d", pg, reads, 38, 2, 0), "8: mode d")
    _check_times(c, "8: mode d", ())
    assert c["searched"] == [reads.shape[0]] * 2


PER_STRAND = ("searched", "candidates", "probes", "entry_fetches", "verifies")
DUAL_OWN = ("dual", "redo_reads", "dual_seed_probes", "dual_skip_reads", "dual_rewinds")


def test_counter_block(case, dual_run, screen_run, plain_run):
    """9. The counters are deterministic: a fresh context under the same knobs counts the same.  And on the reads without
    N, as in tests/test_gpu_parity.py, `searched` and `candidates` are the oracle's restatement of the schedule; the dual
    kernel's own follow from what they count: every read is searched once, a probed seed gathers one or two heads."""
    pg, reads = case["pg"], case["reads"]
    clean = reads[:reads.shape[0] - N_WITH_N]
    o_clean = orc.oracle_match("c", pg, clean, 38, 3, 0)
    pins = {"dual": None, "screened": orc.oracle_match_screened(pg, clean, 38, 3, 0),
            "plain": orc.oracle_match("c", pg, clean, 38, 3, 0, early_stop=True)}
    for name, knobs, (_, c), keys in (("dual", DUAL, dual_run, PER_STRAND + DUAL_OWN), ("screened", SCREEN, screen_run, PER_STRAND),
                                      ("plain", PLAIN, plain_run, PER_STRAND)):
        again = _run(_context(knobs, pg, reads), case["o"], f"9: {name}, a fresh context")
        print(f"\n9: {name}: " + repr({k: c[k] for k in keys}))
        for k in keys:
            assert c[k] == again[k], (name, k, c[k], again[k])
        assert c["screened"] == again["screened"]
        cc = _run(_context(knobs, pg, clean), o_clean, f"9: {name}, reads without N")
        print(f"9: {name}, reads without N: " + repr({k: cc[k] for k in PER_STRAND + DUAL_OWN}))
        if pins[name] is not None:
            assert_same_results(pins[name], o_clean, f"9: {name}: the oracle's restatement of the schedule")
            assert cc["searched"] == pins[name]["searched"] and cc["candidates"] == pins[name]["candidates"], name
        else:
            n = clean.shape[0]
            assert cc["dual"]["searched"] == n
            assert 0 < cc["dual_seed_probes"] <= cc["dual"]["probes"] <= 2 * cc["dual_seed_probes"]
            assert cc["redo_reads"] <= n // 4 + 50 and cc["dual_skip_reads"] <= n
