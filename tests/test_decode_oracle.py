"""The read rebuild on the CPU: decode_util's restatement of the reference decoder's writers (SE, PE, ORD) over the compiled
reference's own export streams gives back the input reads.  HQ list: exportMatchesInPgOrder / exportMatchesInOriginalOrder
of the reference; LQ and N texts: the unmatched reads.  The expected answer is the reads themselves:
  - a matched read's entry decodes to the read that carries its original index,
  - an entry of the old list decodes to its Pg window, reverse-complemented where list_rc is set,
  - LQ and N rows decode to their reads.
Orientation rule that results (and is asserted): in file 2 of PE / ORD order the LQ and N rows are reverse-complemented;
the HQ rows are too exactly when the pair-file rule (revComplPairFile) is on."""
import numpy as np
import pytest

import decode_util as du
import export_util as xu
import oracle as orc

needs_ref = pytest.mark.skipif(not orc.have_adapter(), reason="oracle/_ref not built")

CASES = {
    "se": dict(seed=31, G=120_000, n=5000, n_with_n=150, dups=200),
    "pe_pairfile": dict(seed=32, G=120_000, n=5000, n_with_n=150, dups=200, paired=True),
    "L250": dict(seed=33, G=150_000, n=2500, L=250, n_with_n=60, dups=60, list_gap=110),
}
_cache = {}


def _job(tmp_path, name):
    if name in _cache:
        return _cache[name]
    kw = dict(CASES[name])
    pair = kw.pop("paired", False)
    case = du.close_list(xu.export_case(paired=pair, **kw))
    kmax = case["L"] // 3
    res = orc.ref_match("c", case["pg"], case["reads"], 38, kmax, 0, n_nset=case["n_n"])
    pg_b = xu.ref_export_run(case, str(tmp_path / "p"), 0, kmax=kmax, pair_file_mode=pair, rev_compl_pair_file=pair)
    org_b = xu.ref_export_run(case, str(tmp_path / "o"), 0, kmax=kmax, preserve_order=True, pair_file_mode=pair,
                              rev_compl_pair_file=pair)
    _cache[name] = (case, res, du.streams_from_bytes(pg_b), du.streams_from_bytes(org_b), pair)
    return _cache[name]


@needs_ref
@pytest.mark.parametrize("wide", [False, True], ids=["off8", "off16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_restated_writers_give_back_the_reads(tmp_path, name, wide):
    case, res, pg_st, org_st, pair = _job(tmp_path, name)
    dc = du.decode_case(case, res, pg_st, org_st, pair=pair, wide=wide)
    assert dc["lists"][0]["n"] > 1000 and dc["lists"][1]["n"] > 0 and dc["lists"][2]["n"] > 0
    assert pg_st["mis_cnt"].astype(np.int64).sum() > 100            # mismatches are exercised
    if not pair:
        # SE: HQ entries in Pg order, then LQ, then N (an archive made under the pair-file rule has mismatch lists in
        # the orientation of file 2 for the odd indexes: only PE / ORD decode it)
        se = du.write_se(dc)
        assert np.array_equal(se, du.truth_rows_se(dc, pg_st, case, res))
        # the matched reads' entries are their reads, the old list's entries their (RC'd) Pg windows
        org = pg_st["org_idx"].astype(np.int64)
        owner = np.full(case["total"], -1, np.int64)
        owner[case["read_org"]] = np.arange(case["reads"].shape[0])
        m = owner[org] >= 0
        assert m.sum() > 1000 and (~m).sum() > 100
        assert np.array_equal(se[: org.size][m, :-1], case["reads"][owner[org[m]]])
    # PE: both files from rlIdxOrder
    f1, f2 = du.write_pe(dc, dc["rl_idx_order"], pair)
    assert np.array_equal(f1, du.truth_rows_pe(dc, 0)) and np.array_equal(f2, du.truth_rows_pe(dc, 1))
    # ORD: the original-order export
    odc = dict(dc, lists=dc["ord_lists"])
    files = du.write_ord(odc, dc["org2pos"], paired=pair, pair_file=pair)
    for p, f in enumerate(files):
        assert np.array_equal(f, du.truth_rows_ord(dc, dc["text"], p, pair)), p


@needs_ref
@pytest.mark.parametrize("name", sorted(CASES))
def test_archive_symbol_form_under_a_reordered_symbol_order(tmp_path, name):
    """the reference decoder holds exclusive codes under the archive's bases order (code2mismatch after
    reorderSymAndVal): the restated reordering of the export's context codes decodes to the same rows"""
    case, res, pg_st, org_st, pair = _job(tmp_path, name)
    codes, order = du.exclusive_encoding(pg_st["mis_sym"])
    assert order != b"ACGTN" and codes.max() <= 3
    dc = du.decode_case(case, res, pg_st, org_st, pair=pair, archive=True)
    assert dc["lists"][0]["form"] == 0
    if not pair:
        assert np.array_equal(du.write_se(dc), du.truth_rows_se(dc, pg_st, case, res))
    f1, f2 = du.write_pe(dc, dc["rl_idx_order"], pair)
    assert np.array_equal(f2, du.truth_rows_pe(dc, 1))
    files = du.write_ord(dict(dc, lists=dc["ord_lists"]), dc["org2pos"], paired=pair, pair_file=pair)
    assert np.array_equal(files[-1], du.truth_rows_ord(dc, dc["text"], len(files) - 1, pair))


def test_rev_offsets_round_trip_and_exclusive_codes():
    """convertMisRevOffsets2Offsets restated is the inverse of the builder's backward coding; code2mismatch of an
    exclusive code gives back the mismatch symbol (no reference needed)"""
    rng = np.random.default_rng(5)
    L = 100
    cnt = rng.integers(0, 6, size=400).astype(np.uint8)
    offs = np.concatenate([np.sort(rng.choice(L, size=c, replace=False)) for c in cnt]).astype(np.int64)
    rev = du.offsets_to_rev_offsets(cnt, offs, L)
    assert np.array_equal(du.rev_offsets_to_offsets(cnt, rev, L), offs)
    act = rng.integers(0, 4, size=500)
    mis = (act + rng.integers(1, 5, size=500)) % 5
    ctx = ((act << 4) | mis).astype(np.uint8)
    codes, order = du.exclusive_encoding(ctx)
    got = du.code2mismatch(np.frombuffer(du.ACGTN, np.uint8)[act], codes, order)
    assert np.array_equal(got, np.frombuffer(du.ACGTN, np.uint8)[mis])
