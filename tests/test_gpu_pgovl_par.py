"""The overlap search on the device under the rule of the parallel generator (pgrc_ovl_set_rule; pgrc_amd/csrc/pgovl.hip,
DESIGN.md 4.18): device == the reference-made fixtures of tests/golden/make_golden_pgovl_par.py byte for byte with the recorded
order -- nextRead, overlap, the logged reads-left numbers, the both-sides flags -- and == tests/pgovl_par_util's literal loops
with the order made on the device; the rule info; the serial rule's fixtures on a context that was under the parallel rule in
between; the graph handed to the assembler on the device; one generated set whose first sweeps span several tiles of the
device scan with block starts inside the tiles; one hand-made set whose last read is still without a successor at sweep L - 3,
where compares run past the last row; the parameter errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pgovl_par_util as pp
import pgovl_util as po
import test_pgovl_oracle as serial
from pgrc_amd import OverlapFinder, PgAssembler, PgrcMatchError
from pgrc_amd import _lib
from pgrc_amd._lib import lib
from test_pgovl_oracle import assert_result
from test_pgovl_par_oracle import FIXTURES, case_name, load_case

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = 1, 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [case_name(p) for p in FIXTURES].index("lowcomp_acgt_L12") if FIXTURES else 0


def scan_tile():
    """SCO_EPB of scanops.h: elements of one block of the device scan"""
    text = open(os.path.join(ROOT, "pgrc_amd", "csrc", "scanops.h")).read()
    tpb, ept = (int(re.search(r"#define %s (\d+)" % k, text).group(1)) for k in ("SCO_TPB", "SCO_EPT"))
    return tpb * ept


def rows_of(codes, symbols):
    return po.pack_rows(po.ascii_of(codes, symbols), symbols)


def assert_info(ovl, symbols, L, coef, counters):
    info = ovl.rule_info()
    assert info == {"rule": "parallel", "blocks": symbols ** 3, "tail_sweeps": pp.tail_sweeps(L, coef),
                    "follower_compares": counters["follower_compares"], "past_end_compares": counters["past_end_compares"]}, info
    return info


@pytest.mark.parametrize("path", FIXTURES, ids=case_name)
def test_reference_fixtures(path):
    fx = load_case(path)
    L, symbols, coef = int(fx["L"]), int(fx["symbols"]), float(fx["coef"])
    R = fx["rows"].shape[0]
    ovl = OverlapFinder(device=0)
    got = ovl.run(fx["rows"], L, symbols, coef, fx["sorted_order"], rule="parallel")
    assert got["next_read"].tobytes() == fx["next_read"].tobytes() and got["overlap"].tobytes() == fx["overlap"].tobytes()
    assert got["reads_left"].tobytes() == fx["reads_left"].tobytes()
    assert ovl.both_sides().tobytes() == fx["flags"].tobytes()
    assert got["duplicates"] == R - int(fx["reads_left"][0]) and got["links"] == int(fx["reads_left"][0]) - int(fx["reads_left"][-1])
    assert got["sweeps"] == fx["reads_left"].size - 1
    assert assert_info(ovl, symbols, L, coef, fx["form"]["counters"])["past_end_compares"] == 0
    t = ovl.timing()
    assert t["bytes_down"] == 5 * (R + 1) and t["passes"] <= got["sweeps"] and len(t["ms_sweeps_device"]) == got["sweeps"]
    # the order made on the device: equal reads in ascending number (the rule holds for the later runs of the context)
    order = po.stable_order(fx["codes"])
    lit = pp.literal(fx["codes"], order, coef, symbols)
    again = ovl.run(fx["rows"], L, symbols, coef, None)
    assert_result(again, lit, "own order")
    assert np.array_equal(ovl.both_sides(), po.both_sides(lit["next_read"], lit["overlap"], L))
    if L <= 40:                                             # (the counters of the array form: some seconds of Python at L = 150)
        assert_info(ovl, symbols, L, coef, pp.parallel_form(fx["codes"], order, coef, symbols)["counters"])
    ovl.close()


def test_the_serial_fixtures_pass_after_the_rule_was_parallel_and_back():
    ovl = OverlapFinder(device=0)
    par = load_case(FIXTURES[SMALL])
    for path in serial.FIXTURES:
        fx = serial.load_case(path)
        L, symbols, coef = int(fx["L"]), int(fx["symbols"]), float(fx["coef"])
        ovl.run(par["rows"], int(par["L"]), int(par["symbols"]), float(par["coef"]), par["sorted_order"], rule="parallel")
        assert ovl.rule_info()["rule"] == "parallel"
        got = ovl.run(fx["rows"], L, symbols, coef, fx["sorted_order"], rule="serial")
        assert got["next_read"].tobytes() == fx["next_read"].tobytes() and got["overlap"].tobytes() == fx["overlap"].tobytes()
        assert got["reads_left"].tobytes() == fx["reads_left"].tobytes()
        assert ovl.both_sides().tobytes() == fx["flags"].tobytes()
        assert ovl.rule_info() == {"rule": "serial", "blocks": 0, "tail_sweeps": 0, "follower_compares": 0, "past_end_compares": 0}
    ovl.close()


@pytest.mark.parametrize("symbols", [4, 5])
def test_assemble_equals_the_assembler_on_the_downloaded_arrays(symbols):
    rng = np.random.default_rng(120 + symbols)
    L = 41
    codes = po.gen_mixed(rng, 3000, L, symbols)
    rows = rows_of(codes, symbols)
    ovl, asm, asm2 = OverlapFinder(device=0), PgAssembler(device=0), PgAssembler(device=0)
    ovl.set_rule("parallel")
    for width, mapping in ((1, None), (2, rng.permutation(3000).astype(np.uint32))):
        got = ovl.run(rows, L, symbols, 1.0, None, overlap_width=width)
        assert ovl.rule_info()["tail_sweeps"] == 3
        want = asm2.run(rows, got["next_read"], got["overlap"], L, symbols, mapping)
        mine = ovl.assemble(asm, mapping)
        for k in ("pg_len", "cycles", "overlap_lost", "components", "singles"):
            assert int(mine[k]) == int(want[k]), k
        assert mine["org_idx"].tobytes() == want["org_idx"].tobytes() and mine["off"].tobytes() == want["off"].tobytes()
        assert asm.text().tobytes() == asm2.text().tobytes() and asm.pg_len == want["pg_len"] < 3000 * L
    for x in (ovl, asm, asm2):
        x.close()


def test_first_sweeps_span_several_scan_tiles_with_block_starts_inside():
    """L = 24, ACGNT.  The segmented scan can only go wrong where a block of suffixes starts inside a tile of the scan and where
    the carried order crosses tiles: more than two tiles of suffixes in each of the first three sweeps, 125 blocks, so a block
    start every hundred places or so."""
    tile = scan_tile()
    R = 4 * tile + tile // 3 + 7
    rng = np.random.default_rng(2400)
    codes = po.gen_genome(rng, R, 24, 5, coverage=12.0, subst=0.02, dup=0.02)
    order = po.shuffled_order(rng, codes)
    lit = pp.literal(codes, order, 1.0, 5)
    assert lit["reads_left"][2] > 2 * tile                   # sweeps 1, 2 and 3 merge more than two tiles
    ovl = OverlapFinder(device=0)
    got = ovl.run(rows_of(codes, 5), 24, 5, 1.0, order, rule="parallel")
    assert_result(got, lit, "tiles")
    assert np.array_equal(ovl.both_sides(), po.both_sides(lit["next_read"], lit["overlap"], 24))
    assert not same_graph(lit, po.literal(codes, order, 1.0, 5))    # (the serial rule gives another graph here)
    ovl.close()


def same_graph(a, b):
    return np.array_equal(a["next_read"], b["next_read"]) and np.array_equal(a["overlap"], b["overlap"])


def test_the_last_read_is_without_a_successor_at_sweep_L_minus_3():
    """ACGGT, GGTCC, AAGGT: nothing links at sweep 1; at sweep 2 = L - 3 the block GGT holds read 3 (group A) and read 1 (group
    C), and the merge compares them by the rows behind them -- there is none behind read 3.  The missing row is the smaller:
    read 3 comes first and takes GGTCC.  Not compared with the reference, which reads memory that is not its own here."""
    codes = po.to_codes(np.frombuffer(b"ACGGTGGTCCAAGGT", dtype=np.uint8).reshape(3, 5), 4)
    order = po.stable_order(codes)
    form = pp.parallel_form(codes, order, 1.0, 4)
    assert form["counters"]["past_end_compares"] == 2 == form["counters"]["follower_compares"]
    ovl = OverlapFinder(device=0)
    for so in (order, None):
        got = ovl.run(rows_of(codes, 4), 5, 4, 1.0, so, rule="parallel")
        info = assert_info(ovl, 4, 5, 1.0, form["counters"])
        assert info["past_end_compares"] > 0
        assert pp.valid_graph(codes, got["next_read"], got["overlap"])
        assert got["next_read"].tolist() == [0, 0, 0, 2] and got["overlap"].tolist() == [0, 0, 0, 3]
        assert_result(got, form, "past the end")
    ovl.close()


def test_parameter_errors_leave_the_context_usable():
    fx = load_case(FIXTURES[SMALL])
    L, symbols, coef = int(fx["L"]), int(fx["symbols"]), float(fx["coef"])
    ovl = OverlapFinder(device=0)
    info = _lib.OvlRuleInfo(C.sizeof(_lib.OvlRuleInfo))
    assert lib.pgrc_ovlrule_get_info(ovl._h, C.byref(info)) == E_STATE            # no run yet
    for bad in (2, 3, 0xFFFFFFFF):
        assert lib.pgrc_ovlrule_set(ovl._h, bad) == E_PARAM
        assert (lib.pgrc_ovl_last_error(ovl._h) or b"").decode().startswith("overlap: ")
    got = ovl.run(fx["rows"], L, symbols, coef, fx["sorted_order"])          # a refused value changes nothing: still the serial rule
    assert ovl.rule_info()["rule"] == "serial"
    assert_result(got, po.literal(fx["codes"], fx["sorted_order"], coef, symbols), "serial")
    ovl.set_rule("parallel")
    short = np.random.default_rng(5).integers(0, 4, size=(50, 3)).astype(np.uint8)
    for ll in (1, 2, 3):
        with pytest.raises(PgrcMatchError) as ex:
            ovl.run(rows_of(short[:, :ll], 4), ll, 4, 1.0, None)
        assert ex.value.code == E_PARAM and "at least 4" in str(ex.value)
        with pytest.raises(PgrcMatchError) as ex:               # a refused run leaves no graph and no info behind
            ovl.rule_info()
        assert ex.value.code == E_STATE
        got = ovl.run(fx["rows"], L, symbols, coef, fx["sorted_order"])
        assert got["next_read"].tobytes() == fx["next_read"].tobytes()
    wrong = _lib.OvlRuleInfo(C.sizeof(_lib.OvlRuleInfo) - 8)
    assert lib.pgrc_ovlrule_get_info(ovl._h, C.byref(wrong)) == E_PARAM and lib.pgrc_ovlrule_get_info(ovl._h, None) == E_PARAM
    ovl.set_rule("serial")
    assert_result(ovl.run(rows_of(short, 4), 3, 4, 1.0, None), po.literal(short, po.stable_order(short), 1.0, 4), "L = 3 under the serial rule")
    ovl.close()
