"""pgrc_amd.archive on the host: every framing case through writer and reader, the refusal of a stream nobody can decode, whole
archives of made-up parts in the four modes, and the golden archive: the raw streams a device run recorded
(tests/golden/make_golden_archive.py), assembled here and decoded by the compiled reference."""
import io
import os
import struct
import zlib

import numpy as np
import pytest

import archive_util as au
from pgrc_amd import archive as ar

FAKE = 200                                                      # a coder type the reference does not have


def fake_coder(name, data):
    return FAKE, zlib.compress(data, 9)


def fake_decoder(ctype, payload, dest_len):
    return zlib.decompress(payload) if ctype == FAKE else None


def framed(name, data, coder=None) -> bytes:
    out = io.BytesIO()
    ar.write_stream(out, name, data, coder)
    return out.getvalue()


def reader(raw: bytes, decoder=None) -> ar.StreamReader:
    return ar.StreamReader(io.BytesIO(raw), decoder)


def book() -> bytes:
    from pgrc_amd.pipeline import default_book
    return default_book()


# ------------------------------------------------------------------------------------------------ the framing
def test_an_empty_stream_is_a_lone_zero_length():
    raw = framed("s", b"")
    assert raw == struct.pack("<Q", 0)
    r = reader(raw + raw)
    assert r.read("a") == b"" and r.read("b") == b"" and r.at_end()


def test_a_raw_stream():
    data = bytes(range(256)) * 3
    raw = framed("s", data)
    assert raw == struct.pack("<QQB", len(data), len(data), ar.NO_CODER) + data
    assert reader(raw).read("s") == data
    assert reader(framed("s", np.arange(5, dtype=np.uint32))).read("s") == np.arange(5, dtype=np.uint32).tobytes()


def test_a_coder_that_shrinks_the_stream_and_one_that_does_not():
    data = b"ACGT" * 500
    raw = framed("s", data, fake_coder)
    dest_len, src_len, ctype = struct.unpack("<QQB", raw[:17])
    assert (dest_len, ctype) == (len(data), FAKE) and src_len == len(raw) - 17 < len(data)
    assert reader(raw, fake_decoder).read("s") == data
    noise = np.random.default_rng(1).integers(0, 256, size=300, dtype=np.uint8).tobytes()
    assert framed("s", noise, fake_coder) == framed("s", noise)                    # what does not shrink is stored (writeHeader)
    assert framed("s", data, lambda name, d: None) == framed("s", data)             # a coder may pass
    names = []
    framed("pgs.lengths", data, lambda name, d: names.append(name))
    assert names == ["pgs.lengths"]


@pytest.mark.parametrize("secondary", [None, fake_coder])
def test_the_compound_form_with_the_var_len_book(secondary):
    v = ar.VarLenCoded(book(), bytes([7, 9, 200, 3] * 300), 3100)
    raw = framed("pgs.mapped", v, secondary)
    dest_len, inner_len, ctype, comp_len, primary = struct.unpack("<QQBQB", raw[:26])
    comp = v.to_bytes()
    assert comp[:2] == b"\0\0" and comp[2:2 + len(book()) + 1] == book() + b"\0"   # mode, book id, the book as a C string
    assert (dest_len, ctype, comp_len, primary) == (3100, ar.COMPOUND_CODER_TYPE, len(comp), ar.VARLEN_DNA_CODER)
    assert inner_len == len(raw) - 26                                               # the inner stream with its 17 header bytes
    inner_dest, inner_src, inner_type = struct.unpack("<QQB", raw[26:43])
    assert inner_dest == comp_len and inner_src == inner_len - ar.STREAM_HEADER_LEN
    assert inner_type == (ar.NO_CODER if secondary is None else FAKE)
    got = reader(raw, fake_decoder).read("pgs.mapped")
    assert isinstance(got, ar.VarLenCoded) and got == v and got.book == book() and len(got) == 3100
    assert framed("pgs.mapped", ar.VarLenCoded(book(), b"", 0)) == struct.pack("<Q", 0)


def test_a_collective_block_of_several_jobs():
    jobs = [("a", b"abc"), ("b", b""), ("c", b"x" * 1000), ("d", ar.VarLenCoded(book(), b"\1\2\3", 9)), ("e", np.arange(7, dtype=np.int16))]
    out = io.BytesIO()
    ar.write_collective(out, jobs, fake_coder)
    assert out.getvalue() == b"".join(framed(n, d, fake_coder) for n, d in jobs)    # the jobs' streams one after the other
    r = reader(out.getvalue(), fake_decoder)
    got = r.read_collective([n for n, _ in jobs])
    assert got[:3] == [b"abc", b"", b"x" * 1000] and got[3] == jobs[3][1] and got[4] == jobs[4][1].tobytes() and r.at_end()


def test_a_stream_of_an_unknown_coder_type_is_refused_by_name():
    raw = framed("order.base_pos", b"ACGT" * 500, fake_coder)
    with pytest.raises(ar.ArchiveError, match=r"stream 'order\.base_pos' is coded with coder type 200 \(unknown\) and no decoder was given"):
        reader(raw).read("order.base_pos")
    with pytest.raises(ar.ArchiveError, match=r"stream 'x': the decoder has no coder of type 200"):
        reader(raw, lambda t, p, n: None).read("x")
    lz = struct.pack("<QQB", 10, 4, ar.LZMA_CODER) + b"abcd"
    with pytest.raises(ar.ArchiveError, match=r"stream 'hq\.props' is coded with coder type 1 \(LZMA\)"):
        reader(lz).read("hq.props")
    with pytest.raises(ar.ArchiveError, match="the decoder of type 1 gave 3 bytes for 10"):
        reader(lz, lambda t, p, n: b"abc").read("s")
    with pytest.raises(ar.ArchiveError, match="ends inside the stream"):
        reader(lz[:-1]).read("s")


# ------------------------------------------------------------------------------------------------ whole archives
def made_up_parts(mode: int) -> dict:
    rng = np.random.default_rng(mode)
    L, n = 50, [40, 12, 3]

    def u8(k, hi=256):
        return rng.integers(0, hi, size=k, dtype=np.uint8)
    ord_mode, paired = mode in ar.ORD_MODES, mode in ar.PAIRED_MODES
    T = sum(n) + (sum(n) & 1)
    n[2] += T - sum(n)
    parts = {"mode": mode, "read_length": L, "rev_compl_pair_file": mode in (ar.PGRC_PE_MODE, ar.PGRC_ORD_PE_MODE), "separate_n": True,
             "name": "some_name"}
    for w, k in zip(ar.LISTS, n):
        parts[w] = {"n_entries": k, "pg_length": 900 + k, "off": None if ord_mode else u8(k)}
    dests = [np.zeros(0, np.uint8), u8(9, L), u8(8, L), np.zeros(0, np.uint8), u8(4, L)]
    parts["hq"].update(rev_comp=u8(n[0], 2), archive={"zero_flags": u8(n[0], 2), "nonzero_cnt": u8(15, 5), "mis_sym": u8(21, 4), "bases_order": b"GANTC",
                                                      "props": np.array([4, 1, 2, 3], np.uint8), "dests": dests})
    if mode == ar.PGRC_ORD_SE_MODE:
        parts["order"] = {"positions": rng.integers(0, 2000, size=T, dtype=np.uint32)}
    elif mode == ar.PGRC_ORD_PE_MODE:
        parts["order"] = {k: rng.integers(0, 100, size=5).astype(ar.PAIRPOS_DTYPES.get(k, np.uint32)) for k in ar.PAIRPOS_NAMES}
    elif paired:
        parts["order"] = {k: rng.integers(0, 100, size=6).astype(ar.PAIRORDER_DTYPES[k]) for k in ar.PAIRORDER_NAMES + ar.PAIRORDER_FLAG_NAMES}
    parts["pgs"] = {"mapped_lens": (700, 200, 30), "mapped": ar.VarLenCoded(book(), u8(400), 930), "map_off": [u8(16), u8(4), b""],
                    "map_len": [u8(5), u8(2), b"\x2d"]}
    return parts


@pytest.mark.parametrize("mode", [ar.PGRC_SE_MODE, ar.PGRC_PE_MODE, ar.PGRC_ORD_SE_MODE, ar.PGRC_ORD_PE_MODE])
@pytest.mark.parametrize("coder", [None, fake_coder], ids=["raw", "coded"])
def test_an_archive_of_made_up_parts_reads_back(tmp_path, mode, coder):
    parts = made_up_parts(mode)
    path = str(tmp_path / "a.pgrc")
    size = ar.write_archive(path, parts, coder)
    raw = open(path, "rb").read()
    assert size == len(raw) and not os.path.exists(path + ".temp")
    head = b"PgRC#" + bytes([2, 0, 2, ar.CODER_LEVEL_NORMAL, mode, 1]) + (b"\1" if mode in (ar.PGRC_PE_MODE, ar.PGRC_ORD_PE_MODE) else b"")
    assert raw.startswith(head + b"some_name\nGANTC")
    got = ar.read_archive(path, fake_decoder if coder else None)
    assert (got["mode"], got["read_length"], got["rev_compl_pair_file"], got["name"], got["version"]) == \
        (mode, 50, parts["rev_compl_pair_file"], "some_name", (2, 0, 2))
    assert got["n_total"] == sum(parts[w]["n_entries"] for w in ar.LISTS)
    for w in ar.LISTS:
        assert (got[w]["n_entries"], got[w]["pg_length"]) == (parts[w]["n_entries"], parts[w]["pg_length"])
        assert (got[w]["off"] is None) == (mode in ar.ORD_MODES) and (got[w]["off"] is None or np.array_equal(got[w]["off"], parts[w]["off"]))
    a, b = got["hq"]["archive"], parts["hq"]["archive"]
    assert np.array_equal(got["hq"]["rev_comp"], parts["hq"]["rev_comp"]) and a["bases_order"] == b"GANTC"
    assert all(np.array_equal(a[k], b[k]) for k in ("zero_flags", "nonzero_cnt", "mis_sym", "props"))
    assert len(a["dests"]) == 5 and all(np.array_equal(x, y) for x, y in zip(a["dests"], b["dests"]))
    if parts.get("order") is None:
        assert got["order"] is None
    else:
        for k, v in parts["order"].items():
            assert got["order"][k].dtype == v.dtype and np.array_equal(got["order"][k], v), k
    g, h = got["pgs"], parts["pgs"]
    assert g["mapped_lens"] == h["mapped_lens"] and g["mapped"] == h["mapped"]
    assert all(ar._b(x) == ar._b(y) for x, y in zip(g["map_off"] + g["map_len"], h["map_off"] + h["map_len"]))
    assert got["bytes_left"] == 0
    if coder is None:                                           # without a decoder the coded archive is refused at its first coded stream
        return
    with pytest.raises(ar.ArchiveError, match=r"stream 'hq\.props' is coded with coder type 200"):
        ar.read_archive(path)


def test_what_is_no_archive_is_refused(tmp_path):
    path = str(tmp_path / "x")
    for raw, why in ((b"", "header is missing"), (b"PgRX#", "header is missing"), (b"PgRC\0rest", "before version 1.2"),
                     (b"PgRC#" + bytes([3, 0, 0, 2, 0, 1]), "newer PgRC version 3.0"), (b"PgRC#" + bytes([1, 2, 0, 2, 0, 1]), "1.3 and later"),
                     (b"PgRC#" + bytes([2, 0, 2, 2, 7, 1]), "unsupported decompression mode: 7"), (b"PgRC#" + bytes([2, 0, 2, 2, 0, 1]) + b"name", "ends inside its header"),
                     (b"PgRC#" + bytes([2, 0, 2, 2, 3, 1]), "ends inside its header"), (b"PgRC#" + bytes([2, 0, 2, 2, 4, 1]) + b"n\n", "PGRC_MIN_PE_MODE")):
        open(path, "wb").write(raw)
        with pytest.raises(ar.ArchiveError, match=why):
            ar.read_archive(path)


def test_the_mode_that_ignores_the_pair_order_is_not_written(tmp_path):
    parts = made_up_parts(ar.PGRC_PE_MODE)
    parts["mode"] = ar.PGRC_MIN_PE_MODE
    with pytest.raises(ar.ArchiveError, match="mode 4 is not written"):
        ar.write_archive(str(tmp_path / "a.pgrc"), parts)
    assert not os.path.exists(str(tmp_path / "a.pgrc"))


def test_pseudogenome_properties_as_the_reference_writes_them():
    raw = ar.pg_props(100, 74, 6705, b"ACGT")
    assert raw == b"PGEN\nSEPARATED_PGEN\n1\n100\n74\n6705\n74\n7400\n1\n100\n100\n4\nACGT\nBIN\n"   # (an LQ list of a reference archive, byte for byte)
    assert ar.parse_pg_props(raw) == {"type": "SEPARATED_PGEN", "read_length": 100, "reads_count": 74, "pg_length": 6705, "symbols": b"ACGT",
                                      "text_mode": False}
    assert ar.parse_pg_props(ar.pg_props(100, 0, 0, b"ACGNT"))["reads_count"] == 0
    with pytest.raises(ar.ArchiveError):
        ar.parse_pg_props(b"\0" * 70, "hq.props")


def test_compress_refuses_what_is_out_of_scope(tmp_path):
    """before the device is touched: PGRC_MIN_PE_MODE and the expert options at other values than the reference's defaults"""
    from pgrc_amd import compress
    src = str(tmp_path / "in.fastq")
    au.write_fastq(src, au.make_reads(8, 40, seed=1, noisy=False))
    for option, value in (("ignore_pair_order", True), ("quality_error_limit_in_promils", 200), ("generator_overlap_threshold", 0.5),
                          ("read_seed_length", 30), ("min_chars_per_mismatch", 4), ("target_pg_match_length", 50)):
        with pytest.raises(NotImplementedError, match=option):
            compress(src, archive=str(tmp_path / "a.pgrc"), **{option: value})
    with pytest.raises(TypeError, match="unknown option"):
        compress(src, archive=str(tmp_path / "a.pgrc"), level=3)
    assert not os.path.exists(str(tmp_path / "a.pgrc"))


def test_the_default_book_is_one_the_reference_accepts():
    """256 codes of one to four symbols, the first a single symbol (VarLenDNACoder::initUsing), every symbol of a mapped text
    with a code of its own and no two of them equal in their low three bits (include/pgrc_varlen.h)"""
    codes = book().split(b"\n")
    assert len(codes) == 256 == len(set(codes)) and codes[0] == b"A" and all(1 <= len(c) <= 4 for c in codes)
    singles = [c for c in codes if len(c) == 1]
    assert sorted(singles) == sorted([b"A", b"C", b"G", b"T", b"N", b"%"])
    low = [c[0] & 7 for c in singles]
    assert len(set(low)) == 6 and 0 not in low


# ------------------------------------------------------------------------------------------------ the golden archive
FIXTURE = os.path.join(au.GOLDEN, "archive_streams.npz")


@pytest.mark.skipif(not au.have_ref(), reason="the compiled reference (oracle/_ref) is not here")
@pytest.mark.parametrize("case,paired,order", [("golden_se", False, False), ("golden_ord_pe", True, True)])
def test_golden_streams_make_an_archive_the_reference_decodes(tmp_path, case, paired, order):
    """the raw streams a device run of compress left for 600 reads of 40 bp (a few with N), assembled by write_archive and
    handed to the compiled reference's decoder: the multiset of reads for SE, line for line in both files for ORD-PE"""
    z = np.load(FIXTURE)
    parts = au.unflatten_parts(z, case)
    reads = z[case + "/reads"]
    assert reads.shape == (600, 40) and (reads == ord("N")).any()
    path = str(tmp_path / "g.pgrc")
    ar.write_archive(path, parts)
    got = au.ref_decode(path, paired, 40)
    want = au.source_files(reads, paired)
    if order:
        assert len(got) == 2 and all(np.array_equal(a, b) for a, b in zip(got, want))
    else:
        assert au.same_multiset(got, want)
    back = ar.read_archive(path)                                # and the reader gives the streams back
    assert back["pgs"]["mapped"] == parts["pgs"]["mapped"] and back["n_total"] == 600


@pytest.mark.skipif(not au.have_ref(), reason="the compiled reference (oracle/_ref) is not here")
@pytest.mark.parametrize("paired,order", [(False, False), (True, False), (False, True), (True, True)], ids=["se", "pe", "ord_se", "ord_pe"])
def test_the_references_own_archives_parse_with_its_coders_plugged_in(tmp_path, paired, order):
    """the compiled reference's encoder at -t 1 on 1000 reads of 100 bp; the reader with the reference's Uncompress as the
    decoder takes every stream to the file's last byte, and the parts say what the source says"""
    reads = au.make_reads(1000, 100, coverage=10, seed=21, paired=paired)
    src, pair = au.write_source(str(tmp_path), reads, paired)
    path = str(tmp_path / "ref.pgrc")
    au.ref_encode(src, pair, path, order)
    with pytest.raises(ar.ArchiveError, match=r"stream 'hq\.[a-z_]+' is coded with coder type \d+ \(.+\) and no decoder was given"):
        ar.read_archive(path)                                   # (the first stream that shrank: the properties, or the one behind them)
    parts = ar.read_archive(path, au.ref_decoder())
    mode = (ar.PGRC_ORD_PE_MODE if paired else ar.PGRC_ORD_SE_MODE) if order else (ar.PGRC_PE_MODE if paired else ar.PGRC_SE_MODE)
    assert (parts["mode"], parts["read_length"], parts["n_total"], parts["rev_compl_pair_file"]) == (mode, 100, 1000, paired)
    assert parts["bytes_left"] == 0 and parts["version"] == ar.PGRC_VERSION and parts["separate_n"]
    hq = parts["hq"]
    assert hq["rev_comp"].size == hq["n_entries"] == hq["archive"]["zero_flags"].size and (hq["off"] is None) == order
    assert hq["archive"]["nonzero_cnt"].size == int((hq["archive"]["zero_flags"] == 0).sum())
    assert sum(d.size for d in hq["archive"]["dests"]) == hq["archive"]["mis_sym"].size == int(hq["archive"]["nonzero_cnt"].sum())
    g = parts["pgs"]
    assert isinstance(g["mapped"], ar.VarLenCoded) and len(g["mapped"].book.split(b"\n")) == 256 and len(g["mapped"]) == sum(g["mapped_lens"])
    assert g["mapped_lens"][0] <= hq["pg_length"] and len(g["map_len"][0]) >= 1
    if mode == ar.PGRC_ORD_SE_MODE:
        assert parts["order"]["positions"].size == 1000
    elif mode == ar.PGRC_ORD_PE_MODE:
        assert parts["order"]["base_pos"].size == parts["order"]["off16_flag"].size == 500
    elif mode == ar.PGRC_PE_MODE:
        assert parts["order"]["off8_flag"].size == 500
