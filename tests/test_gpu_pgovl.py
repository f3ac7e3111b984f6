"""The overlap search on the device (pgrc_ovl_run; pgrc_amd/csrc/pgovl.hip): device == the reference-made fixtures byte for
byte -- nextRead, overlap, the logged reads-left numbers, the both-sides flags; device == tests/pgovl_util's parallel form on
generated cases around the wave, block and scan-block sizes, in both alphabets, at read lengths around the 8- and 32-symbol
words and at the ends of the range, with overlaps of one and two bytes, and on the special shapes (all reads equal, no overlap
at all, periodic reads only, a circle that uses P up in the first sweep, everything dropped in the first sweep, no sweep at
all, 20 000 reads of a genome); the order made on the device; every refusal, each followed by a good run on the same
context; the graph handed to the assembler on the device; and a small run after a large one on one context."""
import ctypes as C

import numpy as np
import pytest

import pgovl_util as po
from pgrc_amd import OverlapFinder, PgAssembler, PgrcMatchError
from pgrc_amd import _lib
from pgrc_amd._lib import lib
from test_pgovl_oracle import FIXTURES, assert_result, case_name, load_case

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = 1, 6
BLOCK = 256                 # OV_TPB of pgovl.hip: threads of a block, one suffix each
SCAN_BLOCK = 4096           # SCO_EPB of scanops.h: elements of one block of the device scan
SMALL = [1, 2, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1]


def rows_of(codes, symbols):
    return po.pack_rows(po.ascii_of(codes, symbols), symbols)


def run_device(ovl, codes, symbols, coef, order, width=1):
    got = ovl.run(rows_of(codes, symbols), codes.shape[1], symbols, coef, order, overlap_width=width)
    assert got["overlap"].dtype == (np.uint8 if width == 1 else np.uint16) and got["next_read"].dtype == np.uint32
    return got


def check(ovl, codes, symbols, coef, order, what, width=1):
    want = po.parallel_form(codes, order, coef)
    got = run_device(ovl, codes, symbols, coef, order, width)
    assert_result(got, want, what)
    assert np.array_equal(ovl.both_sides(), po.both_sides(want["next_read"], want["overlap"], codes.shape[1])), what
    return want


@pytest.mark.parametrize("path", FIXTURES, ids=case_name)
def test_reference_fixtures(path):
    fx = load_case(path)
    L, symbols = int(fx["L"]), int(fx["symbols"])
    ovl = OverlapFinder(device=0)
    got = ovl.run(fx["rows"], L, symbols, float(fx["coef"]), fx["sorted_order"])
    assert got["next_read"].tobytes() == fx["next_read"].tobytes() and got["overlap"].tobytes() == fx["overlap"].tobytes()
    assert got["reads_left"].tobytes() == fx["reads_left"].tobytes()
    assert ovl.both_sides().tobytes() == fx["flags"].tobytes()
    R = fx["rows"].shape[0]
    assert got["duplicates"] == R - int(fx["reads_left"][0]) and got["links"] == int(fx["reads_left"][0]) - int(fx["reads_left"][-1])
    assert got["sweeps"] == fx["reads_left"].size - 1
    t = ovl.timing()
    assert t["bytes_down"] == 5 * (R + 1) and t["passes"] <= got["sweeps"] and len(t["ms_sweeps_device"]) == got["sweeps"]
    if case_name(path) == "no_equal_reads":                 # no two reads are equal: the order made on the device is the reference's
        again = ovl.run(fx["rows"], L, symbols, float(fx["coef"]), None)
        assert again["next_read"].tobytes() == fx["next_read"].tobytes() and again["overlap"].tobytes() == fx["overlap"].tobytes()
        assert again["reads_left"].tobytes() == fx["reads_left"].tobytes()
    ovl.close()


@pytest.mark.parametrize("sizes", [SMALL, [SCAN_BLOCK - 1], [SCAN_BLOCK], [SCAN_BLOCK + 1]], ids=["small", "4095", "4096", "4097"])
@pytest.mark.parametrize("symbols", [4, 5])
@pytest.mark.parametrize("L", [1, 2, 31, 32, 33, 150, 255])
def test_generated_cases_equal_the_parallel_form(L, symbols, sizes):
    ovl = OverlapFinder(device=0)
    for k, R in enumerate(sizes):
        rng = np.random.default_rng(1000 * L + 10 * symbols + R)
        codes = po.gen_mixed(rng, R, L, symbols)
        width = 1 + (k + L + R) % 2
        check(ovl, codes, symbols, 1.0, po.shuffled_order(rng, codes), (L, symbols, R), width)
    ovl.close()


def test_all_reads_equal():
    ovl = OverlapFinder(device=0)
    codes = np.repeat(np.random.default_rng(1).integers(0, 4, size=(1, 37)).astype(np.uint8), 300, axis=0)
    order = np.random.default_rng(2).permutation(300).astype(np.uint32) + 1
    want = check(ovl, codes, 4, 1.0, order, "equal")
    assert want["duplicates"] == 299 and int((want["overlap"] == 37).sum()) == 299
    ovl.close()


def test_no_overlap_at_all():
    ovl = OverlapFinder(device=0)
    rng = np.random.default_rng(3)
    codes = np.unique(np.concatenate([np.ones((700, 1), np.uint8), rng.choice(np.array([0, 2, 3], np.uint8), size=(700, 39))], axis=1), axis=0)
    want = check(ovl, codes, 4, 1.0, po.stable_order(codes), "no overlap")      # C, then no C: no suffix is a prefix
    assert want["links"] == 0 and want["duplicates"] == 0 and not ovl.both_sides().any()
    ovl.close()


def test_periodic_reads_only():
    ovl = OverlapFinder(device=0)
    for symbols, L in ((4, 24), (5, 25)):
        rng = np.random.default_rng(4 + symbols)
        # every phase of every unit once (equal reads would stand between a read and its own prefix), the longer units twice more
        units = [np.array(u, np.uint8) for u in ([0], [1], [2], [0, 1], [0, 0, 1], [0, 1, 1], [0, 1, 0, 0])]
        codes = np.stack([u[(np.arange(L) + ph) % u.size] for u in units for ph in range(u.size)]
                         + [u[(np.arange(L) + ph) % u.size] for u in units[4:] for ph in range(u.size)] * 2)
        want = check(ovl, codes, symbols, 1.0, po.shuffled_order(rng, codes), "periodic")
        assert want["counters"]["self_conflicts"] >= 3
        nx = want["next_read"]
        assert any(nx[nx[i]] == i and nx[i] != i for i in range(1, nx.size) if nx[i])       # a 2-cycle
    ovl.close()


def test_a_circle_uses_the_prefixes_up_in_the_first_sweep():
    ovl = OverlapFinder(device=0)
    rng = np.random.default_rng(6)
    circ = rng.integers(0, 4, size=500).astype(np.uint8)
    codes = circ[(np.arange(500)[:, None] + np.arange(40)[None, :]) % 500]
    shuffled = codes[rng.permutation(500)]
    want = check(ovl, shuffled, 4, 1.0, po.stable_order(shuffled), "circle")
    assert want["reads_left"][1] == 0 and want["links"] == 500
    assert ovl.timing()["passes"] == 1                      # the other 38 sweeps had nothing to do
    ovl.close()


def test_everything_dropped_in_the_first_sweep():
    ovl = OverlapFinder(device=0)
    rng = np.random.default_rng(7)
    codes = np.unique(np.concatenate([np.zeros((600, 1), np.uint8), rng.integers(1, 4, size=(600, 29)).astype(np.uint8)], axis=1), axis=0)
    want = check(ovl, codes, 4, 1.0, po.stable_order(codes), "dropped")     # A, then no A: every suffix is above every prefix
    assert want["links"] == 0 and want["counters"]["dropped"] == codes.shape[0] and ovl.timing()["passes"] == 1
    ovl.close()


def test_a_coefficient_just_above_one_over_L_runs_no_sweep():
    ovl = OverlapFinder(device=0)
    rng = np.random.default_rng(8)
    codes = po.gen_genome(rng, 500, 40, 4)
    coef = 1.0 / 40 + 1e-9
    assert po.iterations(40, coef) == 1
    want = check(ovl, codes, 4, coef, po.shuffled_order(rng, codes), "no sweep")
    got = run_device(ovl, codes, 4, coef, None)
    assert got["sweeps"] == 0 and got["links"] == 0 and got["reads_left"].size == 1 and got["duplicates"] == want["duplicates"] > 0
    assert_result(run_device(ovl, codes, 4, 0.0, None), po.parallel_form(codes, po.stable_order(codes), 0.0), "coef 0")
    ovl.close()


def test_20000_reads_of_a_genome_at_coverage_30():
    ovl = OverlapFinder(device=0)
    rng = np.random.default_rng(9)
    codes = po.gen_genome(rng, 20000, 64, 4, coverage=30.0, subst=0.01, dup=0.02)
    want = check(ovl, codes, 4, 1.0, po.shuffled_order(rng, codes), "genome")
    assert want["links"] > 15000 and want["counters"]["tie_runs_off_symbol_order"] > 100
    ovl.close()


@pytest.mark.parametrize("symbols", [4, 5])
def test_order_made_on_the_device(symbols):
    ovl = OverlapFinder(device=0)
    for k, (R, L) in enumerate([(1, 9), (700, 7), (3000, 40), (9000, 150), (2000, 255)]):      # 9 000: more than one tile of the sort
        rng = np.random.default_rng(50 + 10 * symbols + k)
        codes = po.gen_mixed(rng, R, L, symbols)
        want = po.parallel_form(codes, po.stable_order(codes), 1.0)
        assert_result(run_device(ovl, codes, symbols, 1.0, None, 1 + k % 2), want, (R, L))
    ovl.close()


def raw_run(ovl, rows, L, symbols, coef, order, width=1, n_reads=None, struct_size=None):
    R = rows.shape[0] if n_reads is None else n_reads
    inp = _lib.OvlInput(C.sizeof(_lib.OvlInput) if struct_size is None else struct_size, L, symbols, width, R, coef, rows.ctypes.data_as(C.c_void_p),
                        None if order is None else order.ctypes.data_as(C.c_void_p))
    res = _lib.OvlResult()
    rc = lib.pgrc_ovl_run(ovl._h, C.byref(inp), C.byref(res))
    cleared = not res.next_read and not res.overlap and not res.reads_left_after and res.n_reads == 0
    lib.pgrc_ovl_free_result(C.byref(res))
    return rc, cleared, (lib.pgrc_ovl_last_error(ovl._h) or b"").decode()


def test_every_refusal_is_followed_by_a_good_run():
    rng = np.random.default_rng(10)
    L = 40
    codes = po.gen_mixed(rng, 400, L, 5)
    order = po.shuffled_order(rng, codes)
    rows4 = rows_of(np.minimum(codes, 3), 4)
    rows5 = rows_of(codes, 5)
    want5 = po.parallel_form(codes, order, 1.0)
    ovl = OverlapFinder(device=0)
    with pytest.raises(PgrcMatchError) as ex:
        ovl.both_sides()
    assert ex.value.code == E_STATE
    asm = PgAssembler(device=0)
    with pytest.raises(PgrcMatchError) as ex:
        ovl.assemble(asm)
    assert ex.value.code == E_STATE

    def good():
        assert_result(ovl.run(rows5, L, 5, 1.0, order), want5, "good run")

    good()
    twice = order.copy()
    twice[7] = twice[300]
    zero = order.copy()
    zero[0] = 0
    above = order.copy()
    above[399] = 401
    unsorted = order.copy()
    a = int(np.flatnonzero((codes[order[1:] - 1] != codes[order[:-1] - 1]).any(axis=1))[5])
    unsorted[[a, a + 1]] = unsorted[[a + 1, a]]
    big = rows5.copy()
    big[17, 3] = 125
    tail = rows5.copy()                                     # L = 40: the last byte holds one symbol and two zero digits
    tail[200, -1] += 1
    refusals = [("twice", rows5, L, 5, 1.0, twice, {}), ("zero", rows5, L, 5, 1.0, zero, {}), ("above", rows5, L, 5, 1.0, above, {}),
                ("unsorted", rows5, L, 5, 1.0, unsorted, {}), ("byte >= 125", big, L, 5, 1.0, order, {}), ("digits after L", tail, L, 5, 1.0, None, {}),
                ("read_len 0", rows5, 0, 5, 1.0, order, {}), ("read_len 256", rows5, 256, 5, 1.0, order, {}), ("symbols 3", rows5, L, 3, 1.0, order, {}),
                ("width 3", rows5, L, 5, 1.0, order, {"width": 3}), ("no reads", rows5, L, 5, 1.0, order, {"n_reads": 0}),
                ("too many reads", rows5, L, 5, 1.0, order, {"n_reads": 0xFFFFFFFF}), ("coef < 0", rows5, L, 5, -0.1, order, {}),
                ("coef > 1", rows5, L, 5, 1.5, order, {}), ("coef nan", rows5, L, 5, float("nan"), order, {}),
                ("struct_size", rows5, L, 5, 1.0, order, {"struct_size": C.sizeof(_lib.OvlInput) - 8})]
    for what, rows, ll, symbols, coef, so, kw in refusals:
        rc, cleared, msg = raw_run(ovl, rows, ll, symbols, coef, so, **kw)
        assert rc == E_PARAM and cleared and msg.startswith("overlap: "), (what, rc, msg)
        with pytest.raises(PgrcMatchError) as ex:           # a refused run leaves no graph behind
            ovl.both_sides()
        assert ex.value.code == E_STATE, what
        good()
    inp = _lib.OvlInput(C.sizeof(_lib.OvlInput), L, 5, 1, 400, 1.0, None, None)
    res = _lib.OvlResult()
    assert lib.pgrc_ovl_run(ovl._h, C.byref(inp), C.byref(res)) == E_PARAM and lib.pgrc_ovl_run(ovl._h, None, C.byref(res)) == E_PARAM
    assert lib.pgrc_ovl_run(ovl._h, C.byref(inp), None) == E_PARAM and lib.pgrc_ovl_both_sides(ovl._h, None) == E_PARAM
    good()
    # a valid order of ACGT rows is still taken after all that
    codes4 = np.minimum(codes, 3)
    assert_result(ovl.run(rows4, L, 4, 1.0, None), po.parallel_form(codes4, po.stable_order(codes4), 1.0), "acgt")
    asm.close()
    ovl.close()


@pytest.mark.parametrize("symbols", [4, 5])
def test_assemble_equals_the_assembler_on_the_downloaded_arrays(symbols):
    rng = np.random.default_rng(20 + symbols)
    L = 41
    codes = po.gen_mixed(rng, 3000, L, symbols)
    rows = rows_of(codes, symbols)
    ovl, asm, asm2 = OverlapFinder(device=0), PgAssembler(device=0), PgAssembler(device=0)
    for width, mapping in ((1, None), (2, rng.permutation(3000).astype(np.uint32))):
        got = ovl.run(rows, L, symbols, 1.0, None, overlap_width=width)
        want = asm2.run(rows, got["next_read"], got["overlap"], L, symbols, mapping)
        mine = ovl.assemble(asm, mapping)
        for k in ("pg_len", "cycles", "overlap_lost", "components", "singles"):
            assert int(mine[k]) == int(want[k]), k
        assert mine["org_idx"].tobytes() == want["org_idx"].tobytes() and mine["off"].tobytes() == want["off"].tobytes()
        assert asm.text().tobytes() == asm2.text().tobytes() and asm.pg_len == want["pg_len"] < 3000 * L
        assert asm.timing()["bytes_up"] == (0 if mapping is None else 4 * 3000)
        if symbols == 4:
            assert asm.packed_device()
    for x in (ovl, asm, asm2):
        x.close()


def test_a_small_run_after_a_large_one_on_one_context():
    ovl = OverlapFinder(device=0)
    rng = np.random.default_rng(30)
    large = po.gen_genome(rng, 30000, 100, 4, coverage=30.0)
    check(ovl, large, 4, 0.5, po.shuffled_order(rng, large), "large")
    small = po.gen_mixed(rng, 70, 33, 5)
    check(ovl, small, 5, 1.0, po.shuffled_order(rng, small), "small", width=2)
    assert_result(run_device(ovl, small, 5, 1.0, None), po.parallel_form(small, po.stable_order(small), 1.0), "small, own order")
    ovl.close()
