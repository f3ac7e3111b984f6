"""The restatement of the Huffman mode (tests/huf_util.py) against the compiled reference (oracle/_ref): what it writes, the
reference's FSEUncompress reads; what HUF_compress2 writes, it reads; and its coded sizes stay within a measured margin of
HUF_compress2's.  The device code is held to the restatement byte for byte (tests/test_gpu_huf.py), so these are the checks of
the format itself.  No GPU."""
import numpy as np
import pytest

import archive_util as au
import huf_util as hu

pytestmark = pytest.mark.skipif(not au.have_ref(), reason="the compiled reference (oracle/_ref) is not here")

KINDS = hu.KINDS + ("mixed",)
# The coded size of a chunk against HUF_compress2's, measured over every chunk of REF_SHAPES x KINDS that both code (CPU,
# against the reference, never against the device code):
#   all chunks        worst 1.1644 ("four" at 4096 bytes: 248 bytes for 213).  The whole difference is the header: this writer
#                     stores the weights of symbols 0 .. 'T' as 43 raw bytes where the reference FSE-codes them into 8
#   chunks >= 64 KiB  worst 1.0410 (the Fibonacci-like counts at 131072 bytes: 47460 bytes for 45592).  That is the length
#                     limit: the free tree is 24 deep, and dropping a longest code and splitting the longest shorter one costs
#                     more there than the reference's repair by cost
# and asserted with an allowance of 0.01 on top.
WORST_ANY, WORST_LARGE, ALLOWANCE = 1.1644, 1.0410, 0.01


def make(kind: str, n: int, order: int) -> np.ndarray:
    return hu.mixed(n, order) if kind == "mixed" else hu.source(kind, n)


@pytest.fixture(scope="module")
def ref_decoder():
    return au.ref_decoder()


@pytest.mark.parametrize("kind", KINDS)
def test_the_reference_reads_what_the_restatement_writes(ref_decoder, kind):
    for order, lengths in hu.REF_SHAPES:
        for n in lengths:
            x = make(kind, n, order)
            for tl in (11, 8):
                f = hu.encode(x, order, tl)
                assert len(f) <= hu.bound(n, order)
                assert ref_decoder(5, f, n) == x.tobytes(), (kind, n, order, tl)
                assert hu.decode(f, n) == x.tobytes(), (kind, n, order, tl)


@pytest.mark.parametrize("kind", KINDS)
def test_the_restatement_reads_what_the_reference_writes(kind):
    """frames assembled from HUF_compress2 per chunk (a chunk it refuses is stored raw), at table logs 11 and 12"""
    for order, lengths in hu.REF_SHAPES:
        for n in lengths:
            x = make(kind, n, order)
            for tl in (11, 12):
                chunks = [hu.ref_compress_chunk(c, tl) or c.tobytes() for c in hu.split(x, order)]
                assert hu.decode(hu.frame(chunks, order, tl), n) == x.tobytes(), (kind, n, order, tl)


@pytest.mark.parametrize("place", [0, 1, 2])
@pytest.mark.parametrize("what", ["raw", "rle"])
def test_hand_made_raw_and_rle_chunks_in_every_place(ref_decoder, place, what):
    x = hu.source("geo", 3 * 1024, seed=4)
    if what == "rle":
        x = x.copy()
        x[place * 1024:(place + 1) * 1024] = 0x55
    chunks = [hu.encode_chunk(c, 11) for c in hu.split(x, 10)]
    assert all(1 < len(c) < 1024 for k, c in enumerate(chunks) if k != place)
    chunks[place] = b"\x55" if what == "rle" else x[place * 1024:(place + 1) * 1024].tobytes()
    f = hu.frame(chunks, 10, 11)
    assert hu.decode(f, x.size) == x.tobytes() and ref_decoder(5, f, x.size) == x.tobytes()


def test_the_coded_size_stays_within_the_measured_margin_of_the_references():
    worst_any, worst_large = (0.0, None), (0.0, None)
    for order, lengths in hu.REF_SHAPES:
        for kind in KINDS:
            for n in lengths:
                for c in hu.split(make(kind, n, order), order):
                    r = hu.ref_compress_chunk(c)
                    ours = hu.chunk_plan(c, 11)[5]
                    if r is None or len(r) == 1:
                        continue
                    ratio = ours / len(r)
                    worst_any = max(worst_any, (ratio, (kind, n, c.size, ours, len(r))))
                    if c.size >= 1 << 16:
                        worst_large = max(worst_large, (ratio, (kind, n, c.size, ours, len(r))))
    print("worst ratio, any chunk:", worst_any, " chunks >= 64 KiB:", worst_large)
    assert worst_any[0] <= WORST_ANY + ALLOWANCE, worst_any
    assert worst_large[0] <= WORST_LARGE + ALLOWANCE, worst_large


def test_the_committed_fixtures_are_the_references_frames(ref_decoder):
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_huf as mg
    for name, order, tl, src, f in hu.load_golden():
        assert mg.ref_frame(src, order, tl) == f, name
        assert ref_decoder(5, f, src.size) == src.tobytes() and hu.decode(f, src.size) == src.tobytes(), name
