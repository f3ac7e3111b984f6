"""pgrc_amd.compress and pgrc_amd.decompress on the MI355X: the four archive modes and two degenerate inputs, each archive
read back (a) by decompress and the device verifier and (b) by the compiled reference's decoder, which knows nothing of this
package; and the reference's own archive, whose coded streams are refused by name."""
import os

import numpy as np
import pytest

import archive_util as au
from pgrc_amd import archive as ar, compress, decompress, pipeline
from pgrc_amd.verify import VERIFY_IN_ORDER, VERIFY_MULTISET

pytestmark = pytest.mark.gpu

L = 100
MODES = {"se": (ar.PGRC_SE_MODE, False, False), "pe": (ar.PGRC_PE_MODE, True, False),
         "ord_se": (ar.PGRC_ORD_SE_MODE, False, True), "ord_pe": (ar.PGRC_ORD_PE_MODE, True, True)}
needs_ref = pytest.mark.skipif(not au.have_ref(), reason="the compiled reference (oracle/_ref) is not here")


@pytest.fixture(scope="module")
def sources():
    """4000 reads of 100 bp, single and paired, made once"""
    return {False: au.make_reads(4000, L, seed=11), True: au.make_reads(4000, L, seed=12, paired=True)}


@pytest.fixture(scope="module")
def archives(sources, tmp_path_factory):
    """every mode's archive, written once by compress: name -> (path, report, reads, paired, order)"""
    out = {}
    for name, (mode, paired, order) in MODES.items():
        d = str(tmp_path_factory.mktemp(name))
        src, pair = au.write_source(d, sources[paired], paired)
        report = compress(src, pair, archive=os.path.join(d, "a.pgrc"), preserve_order=order)
        assert report["mode"] == mode and report["reads"] == 4000 and os.path.getsize(report["archive"]) == report["bytes"]
        out[name] = (report["archive"], report, sources[paired], paired, order)
    return out


def same_reads(got, reads, paired, order) -> bool:
    want = au.source_files(reads, paired)
    if len(got) != len(want):
        return False
    if order:
        return all(np.array_equal(a, b) for a, b in zip(got, want))
    return au.same_multiset(got, want)


def verified(path, reads, paired, order) -> dict:
    """check (a): decompress gives the reads, and the device verifier says the job equals the source"""
    dec, parts = pipeline.load(path)
    try:
        with dec.verifier(VERIFY_IN_ORDER if order else VERIFY_MULTISET) as v:
            for f, rows in enumerate(au.source_files(reads, paired)):
                v.add_rows(f, np.ascontiguousarray(rows))
            res = v.finish()
    finally:
        dec.close()
    assert res["ok"] and res["kind"] == (VERIFY_IN_ORDER if order else VERIFY_MULTISET), res
    assert res["n_decoded"][0] == res["n_source"][0] == reads.shape[0] // (2 if paired else 1)
    rows = decompress(path)
    assert all(r.shape[1] == reads.shape[1] + 1 and (r[:, -1] == ord("\n")).all() for r in rows)
    assert same_reads([r[:, :-1] for r in rows], reads, paired, order)
    return parts


@pytest.mark.parametrize("name", list(MODES))
def test_every_stream_of_the_case_is_filled(archives, name):
    """the size is the smallest at which nothing of the archive is empty: three pseudogenomes, mapping streams for all three,
    an entry with two or more mismatches, and the order streams of the mode"""
    path, report, reads, paired, order = archives[name]
    parts = ar.read_archive(path)
    assert all(report["counts"]) and all(report["pg_lengths"]) and sum(report["counts"]) == 4000
    g = parts["pgs"]
    assert all(len(x) for x in g["map_off"]) and all(len(x) > 1 for x in g["map_len"]) and isinstance(g["mapped"], ar.VarLenCoded)
    assert tuple(g["mapped_lens"]) == report["mapped_lengths"] and sum(g["mapped_lens"]) < sum(report["pg_lengths"])
    a = parts["hq"]["archive"]
    assert a["nonzero_cnt"].max() >= 2 and a["mis_sym"].size > a["nonzero_cnt"].size and len(a["dests"]) - 1 == a["props"][0] >= 2
    assert 0 < int(parts["hq"]["rev_comp"].sum()) < parts["hq"]["n_entries"]
    assert (parts["hq"]["off"] is None) == order and (parts["lq"]["off"] is None) == order
    if name == "pe":
        assert all(parts["order"][k].size for k in ("off8_flag", "off_value", "delta8_flag", "full_offset", "off_base_file_flag"))
    elif name == "ord_se":
        assert parts["order"]["positions"].size == 4000
    elif name == "ord_pe":
        assert all(parts["order"][k].size for k in ("base_pos", "off16_flag", "off_base_first", "off_value"))
    else:
        assert parts["order"] is None


@pytest.mark.parametrize("name", list(MODES))
def test_round_trip_through_decompress_and_the_verifier(archives, name):
    path, report, reads, paired, order = archives[name]
    parts = verified(path, reads, paired, order)
    assert parts["mode"] == report["mode"] and parts["n_total"] == 4000 and parts["rev_compl_pair_file"] == paired


@needs_ref
@pytest.mark.parametrize("name", list(MODES))
def test_the_reference_decodes_what_compress_writes(archives, name):
    """check (b), the one that proves the container: the unmodified reference decoder on the same file"""
    path, report, reads, paired, order = archives[name]
    assert same_reads(au.ref_decode(path, paired, L), reads, paired, order)


def test_decompress_writes_the_files_the_reference_names(archives, tmp_path):
    for name in ("se", "ord_pe"):
        path, _, reads, paired, order = archives[name]
        names = decompress(path, out_prefix=str(tmp_path / name))
        assert [os.path.basename(n) for n in names] == ([name + "_out_1", name + "_out_2"] if paired else [name + "_out"])
        assert same_reads([au.read_rows(n, L) for n in names], reads, paired, order)


@needs_ref
def test_the_references_archive_is_refused_by_its_first_coded_stream(sources, tmp_path):
    src, _ = au.write_source(str(tmp_path), sources[False], False)
    arc = str(tmp_path / "ref.pgrc")
    au.ref_encode(src, None, arc, False)
    with pytest.raises(ar.ArchiveError, match=r"stream 'hq\.props' is coded with coder type 5 \(FSE/Huffman\) and no decoder was given"):
        decompress(arc)
    head = ar.read_header(open(arc, "rb"))
    assert head["mode"] == ar.PGRC_SE_MODE and head["version"] == ar.PGRC_VERSION


def edge_reads(kind: str) -> np.ndarray:
    rng = np.random.default_rng(3)
    if kind == "random":                                        # no two reads overlap, none maps: everything is LQ
        return au.ACGT[rng.integers(0, 4, size=(2000, L))]
    return np.tile(au.ACGT[rng.integers(0, 4, size=L)], (2000, 1))      # every read a duplicate of one read


@pytest.fixture(scope="module")
def degenerate(tmp_path_factory):
    """kind -> (report, reads) of the two degenerate inputs in the SE mode and of the random reads in the PE mode"""
    out = {}
    for kind, paired in (("random", False), ("duplicates", False), ("random", True)):
        d = str(tmp_path_factory.mktemp(kind))
        reads = edge_reads(kind)
        src, pair = au.write_source(d, reads, paired)
        out[(kind, paired)] = (compress(src, pair, archive=os.path.join(d, "a.pgrc")), reads)
    return out


DEGENERATE = [("random", False), ("duplicates", False), ("random", True)]
DEGENERATE_IDS = ["random", "duplicates", "random-pe"]


@pytest.mark.parametrize("kind,paired", DEGENERATE, ids=DEGENERATE_IDS)
def test_degenerate_inputs_still_decode(degenerate, kind, paired):
    report, reads = degenerate[(kind, paired)]
    assert sum(report["counts"]) == 2000
    if kind == "random":
        assert report["counts"] == (0, 2000, 0) and report["pg_lengths"][0] == 0        # the HQ list is empty
    else:
        assert report["counts"][0] > 0 and report["pg_lengths"][0] >= L
    verified(report["archive"], reads, paired, False)


@needs_ref
@pytest.mark.parametrize("kind,paired", DEGENERATE, ids=DEGENERATE_IDS)
def test_the_reference_decodes_the_degenerate_archives(degenerate, kind, paired):
    report, reads = degenerate[(kind, paired)]
    assert same_reads(au.ref_decode(report["archive"], paired, L), reads, paired, False)


@pytest.mark.parametrize("kind,paired,order,why", [("random", False, True, "ORD_SE mode without an HQ pseudogenome"),
                                                   ("random", True, True, "ORD_PE mode without an HQ pseudogenome"),
                                                   ("duplicates", True, False, "PE mode where no read can be mapped"),
                                                   ("duplicates", False, True, "ORD_SE mode where no read can be mapped")])
def test_degenerate_inputs_the_other_modes_refuse(tmp_path, kind, paired, order, why):
    src, pair = au.write_source(str(tmp_path), edge_reads(kind), paired)
    with pytest.raises(NotImplementedError, match=why):
        compress(src, pair, archive=str(tmp_path / "a.pgrc"), preserve_order=order)
    assert not os.path.exists(str(tmp_path / "a.pgrc"))


# ------------------------------------------------------------------------------------------------ the other two text formats
TEXTS = [("fasta", False, False), ("fasta", True, True), ("lines", False, False), ("lines", False, True)]
TEXT_IDS = ["fasta-se", "fasta-ord_pe", "lines-se", "lines-ord_se"]


@pytest.fixture(scope="module")
def text_archives(sources, tmp_path_factory):
    """FASTA and one-read-per-line sources of the same reads, compressed once each"""
    out = {}
    for fmt, paired, order in TEXTS:
        d = str(tmp_path_factory.mktemp(fmt))
        files = au.source_files(sources[paired], paired)
        names = [os.path.join(d, f"in_{k}.{fmt}") for k in range(len(files))]
        for name, rows in zip(names, files):
            au.write_text(name, rows, fmt)
        report = compress(names[0], names[1] if paired else None, archive=os.path.join(d, "a.pgrc"), preserve_order=order)
        out[(fmt, paired, order)] = (report, sources[paired])
    return out


@pytest.mark.parametrize("fmt,paired,order", TEXTS, ids=TEXT_IDS)
def test_fasta_and_one_read_per_line_sources_round_trip(text_archives, fmt, paired, order):
    """no qualities, so no quality division: the divider runs at error limit 1 and every read without an N starts as HQ"""
    report, reads = text_archives[(fmt, paired, order)]
    assert report["reads"] == 4000 and all(report["counts"])
    verified(report["archive"], reads, paired, order)


@needs_ref
@pytest.mark.parametrize("fmt,paired,order", TEXTS, ids=TEXT_IDS)
def test_the_reference_decodes_archives_of_fasta_and_line_sources(text_archives, fmt, paired, order):
    report, reads = text_archives[(fmt, paired, order)]
    assert same_reads(au.ref_decode(report["archive"], paired, L), reads, paired, order)


def test_a_pair_file_beside_one_read_per_line_text_is_refused(sources, tmp_path):
    from pgrc_amd import PgrcMatchError
    names = [str(tmp_path / "a.txt"), str(tmp_path / "b.txt")]
    for name, rows in zip(names, au.source_files(sources[True][:200], True)):
        au.write_text(name, rows, "lines")
    with pytest.raises(PgrcMatchError, match="no pair file"):
        compress(names[0], names[1], archive=str(tmp_path / "a.pgrc"))


# ------------------------------------------------------------------------------------------------ sources in pieces
@pytest.mark.parametrize("name", ["se", "ord_pe"])
def test_a_source_read_in_many_pieces_gives_the_same_archive(archives, tmp_path, monkeypatch, name):
    """pieces of 5000 bytes (about 24 records, none ending where a piece ends), the rest handed over again: byte for byte the
    archive of the source read in one piece"""
    path, _, reads, paired, order = archives[name]
    monkeypatch.setattr(pipeline, "PIECE_BYTES", 5000)
    src, pair = au.write_source(str(tmp_path), reads, paired)
    report = compress(src, pair, archive=str(tmp_path / "a.pgrc"), preserve_order=order)
    assert report["reads"] == 4000 and open(report["archive"], "rb").read() == open(path, "rb").read()


def test_pair_files_of_unequal_length_are_refused(sources, tmp_path, monkeypatch):
    """file 2 lacks its last 300 records: the first file goes on for pieces after the second has ended (final_piece 4) until
    the divider says the reference's iteration is through, one read past the last whole pair (include/pgrc_reads.h); an odd
    number of reads is no paired source"""
    reads = sources[True]
    monkeypatch.setattr(pipeline, "PIECE_BYTES", 5000)
    src, pair = str(tmp_path / "in_1.fastq"), str(tmp_path / "in_2.fastq")
    au.write_fastq(src, reads[0::2])
    au.write_fastq(pair, reads[1::2][:1700])
    with pytest.raises(ValueError, match="3401 reads in two files of unequal length"):
        compress(src, pair, archive=str(tmp_path / "a.pgrc"))
    assert not os.path.exists(str(tmp_path / "a.pgrc"))


# ------------------------------------------------------------------------------------------------ the reference's archives, its coders plugged in
@needs_ref
@pytest.mark.parametrize("name", ["se", "ord_pe"])
def test_the_references_archive_decodes_with_its_coders_plugged_in(archives, tmp_path, name):
    """the compiled reference's encoder at -t 1 on the case's source; decompress with the reference's Uncompress as the decoder
    plug-in gives the reads back, the reference's own var-len book included"""
    _, _, reads, paired, order = archives[name]
    src, pair = au.write_source(str(tmp_path), reads, paired)
    arc = str(tmp_path / "ref.pgrc")
    au.ref_encode(src, pair, arc, order)
    rows = decompress(arc, decoder=au.ref_decoder())
    assert same_reads([r[:, :-1] for r in rows], reads, paired, order)
