"""pgrc_amd.compress with HufCoder plugged in as the container's coder, in the four archive modes: the archive is smaller than
the one written without a coder, decompress with HufCoder's decoder gives the reads back, and so does the unmodified
reference decoder; the archive written without a coder does not change; and the reference's own archive, whose first coded
stream is in FSE mode, is still refused by name unless the reference's coders are plugged in behind HufCoder's."""
import os

import numpy as np
import pytest

import archive_util as au
from pgrc_amd import HufCoder, archive as ar, compress, decompress, pipeline
from pgrc_amd.verify import VERIFY_IN_ORDER, VERIFY_MULTISET

pytestmark = pytest.mark.gpu

L = 100
MODES = {"se": (ar.PGRC_SE_MODE, False, False), "pe": (ar.PGRC_PE_MODE, True, False),
         "ord_se": (ar.PGRC_ORD_SE_MODE, False, True), "ord_pe": (ar.PGRC_ORD_PE_MODE, True, True)}
needs_ref = pytest.mark.skipif(not au.have_ref(), reason="the compiled reference (oracle/_ref) is not here")


@pytest.fixture(scope="module")
def h():
    coder = HufCoder(device=0)
    yield coder
    coder.close()


@pytest.fixture(scope="module")
def sources():
    return {False: au.make_reads(4000, L, seed=11), True: au.make_reads(4000, L, seed=12, paired=True)}


@pytest.fixture(scope="module")
def archives(h, sources, tmp_path_factory):
    """per mode, from ONE run of the stages: the archive without a coder and the one with HufCoder's; and what the plug-in was
    asked and answered: name -> (plain path, coded path, reads, paired, order, [(stream, data bytes, payload bytes)])"""
    out = {}
    for name, (mode, paired, order) in MODES.items():
        d = str(tmp_path_factory.mktemp(name))
        src, pair = au.write_source(d, sources[paired], paired)
        parts, report = pipeline.compress_parts(src, pair, order)
        assert report["mode"] == mode
        asked = []

        def coder(stream, data):
            ctype, payload = h.coder(stream, data)
            asked.append((stream, len(data), len(payload)))
            return ctype, payload
        plain, coded = os.path.join(d, "plain.pgrc"), os.path.join(d, "huf.pgrc")
        assert ar.write_archive(plain, parts, None) == os.path.getsize(plain)
        assert ar.write_archive(coded, parts, coder) == os.path.getsize(coded)
        out[name] = (plain, coded, sources[paired], paired, order, asked, (src, pair))
    return out


def same_reads(got, reads, paired, order) -> bool:
    want = au.source_files(reads, paired)
    if len(got) != len(want):
        return False
    if order:
        return all(np.array_equal(a, b) for a, b in zip(got, want))
    return au.same_multiset(got, want)


@pytest.mark.parametrize("name", list(MODES))
def test_the_coded_archive_is_smaller_and_every_coded_stream_shrank(h, archives, name):
    plain, coded, _, _, _, asked, _ = archives[name]
    assert os.path.getsize(coded) < os.path.getsize(plain)
    seen = []

    def decoder(ctype, payload, dest_len):
        seen.append((ctype, len(payload), dest_len))
        return h.decoder()(ctype, payload, dest_len)
    ar.read_archive(coded, decoder)
    assert seen and all(ctype == ar.FSE_HUF_CODER and size < dest for ctype, size, dest in seen)
    shrank = [a for a in asked if a[2] < a[1]]
    assert len(seen) == len(shrank) and sorted((s, d) for _, s, d in seen) == sorted((p, n) for _, n, p in shrank)
    print(f"{name}: {os.path.getsize(plain)} bytes without a coder, {os.path.getsize(coded)} with HufCoder; "
          f"{len(shrank)} of {len(asked)} streams coded")


@pytest.mark.parametrize("name", list(MODES))
def test_decompress_with_the_plug_in_gives_the_reads_back(h, archives, name):
    _, coded, reads, paired, order, _, _ = archives[name]
    dec, parts = pipeline.load(coded, decoder=h.decoder())
    try:
        with dec.verifier(VERIFY_IN_ORDER if order else VERIFY_MULTISET) as v:
            for f, rows in enumerate(au.source_files(reads, paired)):
                v.add_rows(f, np.ascontiguousarray(rows))
            res = v.finish()
    finally:
        dec.close()
    assert res["ok"], res
    rows = decompress(coded, decoder=h.decoder())
    assert same_reads([r[:, :-1] for r in rows], reads, paired, order)
    with pytest.raises(ar.ArchiveError, match=r"is coded with coder type 5 \(FSE/Huffman\) and no decoder was given"):
        decompress(coded)


@needs_ref
@pytest.mark.parametrize("name", list(MODES))
def test_the_reference_decodes_the_coded_archive(archives, name):
    _, coded, reads, paired, order, _, _ = archives[name]
    assert same_reads(au.ref_decode(coded, paired, L), reads, paired, order)


@pytest.mark.parametrize("name", list(MODES))
def test_the_archive_without_a_coder_is_what_compress_writes(archives, tmp_path, name):
    """the default path does not know the coder: compress without one writes, byte for byte, the container's plain file"""
    plain, _, _, _, order, _, (src, pair) = archives[name]
    report = compress(src, pair, archive=str(tmp_path / "a.pgrc"), preserve_order=order)
    assert open(report["archive"], "rb").read() == open(plain, "rb").read()


@needs_ref
def test_the_references_archive_needs_its_coders_behind_the_plug_in(h, sources, tmp_path):
    """its first coded stream, hq.props, is type 5 in FSE mode: HufCoder's decoder alone hands it on to nobody"""
    src, _ = au.write_source(str(tmp_path), sources[False], False)
    arc = str(tmp_path / "ref.pgrc")
    au.ref_encode(src, None, arc, False)
    with pytest.raises(ar.ArchiveError, match=r"stream 'hq\.props': the decoder has no coder of type 5 \(FSE/Huffman\)"):
        decompress(arc, decoder=h.decoder())
    rows = decompress(arc, decoder=h.decoder(fallback=au.ref_decoder()))
    assert same_reads([r[:, :-1] for r in rows], sources[False], False, False)
